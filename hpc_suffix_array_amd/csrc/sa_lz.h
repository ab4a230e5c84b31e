// sa_lz.h -- the longest previous factor array and the LZ77 factorisation of
// the text (sa_lpf / sa_lpf_device / sa_lz77 / sa_lz77_device of
// include/sa_hip.h).
//
// LPF[i] = the longest l such that T[i .. i + l) occurs at some j < i (the two
// occurrences may overlap); SRC[i] = the canonical such j.  With r the rank of
// suffix i, a the nearest rank below r and b the nearest rank above r whose SA
// entry is smaller than i: LPF[i] = max(min lcp(a + 1 .. r], min lcp(r + 1 ..
// b]), and SRC[i] = SA[a] when the left minimum is positive and at least the
// right one, else SA[b] when the right one is positive, else none.  The text
// is never compared: every length is an LCP range minimum gathered while the
// nearest smaller value is searched, so a^n costs what its n costs.
//
// LPF, three phases:
//   k_lpf_minima   a hierarchy of (min SA, min LCP) pairs with fan-out kLzFan
//                  over the ranks.  One workgroup per tile of kLzTile ranks:
//                  SA and LCP into LDS, the tile's 64 level-1 nodes by
//                  wavefront reductions, its level-2 node from those; both
//                  written to the global hierarchy.
//   k_lpf_reduce   levels 3 and up (n / 64^3 nodes and fewer), one lane per
//                  node, one launch per level.
//   k_lpf_resolve  one workgroup per tile, the tile and its two levels in LDS
//                  again.  A lane walks from its rank to the left and to the
//                  right (lpf_walk_left / lpf_walk_right): a node whose
//                  smallest SA entry is not below the lane's own is skipped
//                  and gives its LCP minimum, which is exact because the
//                  answer lies beyond it; the walk climbs a level whenever
//                  it stands at a node boundary, so it passes at most kLzFan
//                  - 1 nodes per level on the way up and as many on the way
//                  down into the node that holds the answer.  A walk that
//                  leaves the tile goes on in the global hierarchy from the
//                  tile's edge with the minimum it has so far, its nodes
//                  taken kLpfChunk at a time with their loads issued
//                  together (a step costs one latency): that is every
//                  rank's right walk on an ascending SA and about 2 ln(tile)
//                  ranks per tile on random text.  Nothing is sized on
//                  either case.  The results go to text order by lpf[SA[r]]
//                  and src[SA[r]]: two 4-byte scatters, the BWT's access
//                  shape.
//   A fused form (the tile kernel resolving what it can and listing the rest
//   for a second kernel) would read SA and LCP once instead of twice and run
//   the walks that leave their tile densely; DESIGN.md section 15.
//   Every input and output needs 4-byte alignment only: the loads are
//   coalesced dwords, the stores 4-byte vector stores.
//
// LZ77 (greedy, self-referential): phrase starts p0 = 0, p(k+1) = next(p(k)),
// next(i) = i + max(1, LPF[i]).  No thread walks the text:
//   k_lz_exits     per tile of kLzTile positions, next() in LDS and log2(tile)
//                  rounds of pointer jumping: exit[i] = the first position at
//                  or past the tile's end on the path from i.  The table is
//                  written coalesced; position 0 and every distinct exit
//                  below n are marked in a byte mask.
//   candidates     sa_select_u8_device compacts the mask (sizing call, then
//                  the writing one).  A candidate's successor is its exit,
//                  again a candidate or n: k_lz_succ turns it into an index
//                  by a lower bound.  k_lz_reach, ceil(log2(c)) launches:
//                  flag[J[k]] |= flag[k], J = J o J, from flag[0]; after t
//                  rounds the first 2^t candidates of the path from 0 are
//                  flagged.  k_lz_entry: a tile's flagged candidate is where
//                  the parse enters it (a tile has at most one).
//   k_lz_mark      per entered tile: the path's members inside the tile by the
//                  same doubling in LDS; one bit per position, the count per
//                  tile.  scan_i64<ScanSum> over the counts.
//   k_lz_emit      (pos, len, src) at tile base + rank, when z fits out_cap.
//                  It reads z on the device, so it is launched before the
//                  host knows z.
//
// Host waits per call.  sa_lpf_device with d_lcp: none (it only enqueues);
// without: sa_lcp_device's own.  sa_lz77_device: three (the candidate count,
// the candidate list, z).
//
// The walks, next(), the jump and reach steps compile on the host:
// tests/cpp/lz_check.cpp checks them against the O(n^2) definition and the
// serial parse.  Measurements and the resource report: DESIGN.md section 15.
// The HIP part needs sa_host.h, sa_locate.h (LocBuf), sa_query.h
// (mem_block_excl) and sa_build.hip's scan_i64 and lcp_device before it.
#pragma once
#include <stdint.h>

#include "sa_search.h"   // SA_HD

// (the host compiler of the check program does not know the pragma)
#if defined(__clang__)
#define SA_LZ_UNROLL _Pragma("unroll")
#else
#define SA_LZ_UNROLL
#endif

namespace sa {

constexpr uint32_t kLpfNone = 0xFFFFFFFFu;   // = SA_LPF_NONE
constexpr uint32_t kLzFan = 64;              // children per node of the hierarchy
constexpr uint32_t kLzTile = 4096;           // ranks (LPF) or positions (parse) per workgroup: two levels
constexpr int kLpfMaxLevels = 7;             // 64^6 > 2^32: level 6 is one node

// (smallest SA entry, smallest LCP entry) of a node; level 0: the entries themselves
struct LpfNode {
    uint32_t sa, lcp;
};

SA_HD uint32_t lz_min32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// nodes per level, up to the level that is one node: cnt[0] = n; returns the
// number of levels (1 for n <= 1)
template <uint32_t F>
SA_HD int lpf_level_counts(uint64_t n, uint64_t (&cnt)[kLpfMaxLevels]) {
    cnt[0] = n;
    int levels = 1;
    while (levels < kLpfMaxLevels && cnt[levels - 1] > 1) {
        cnt[levels] = (cnt[levels - 1] + F - 1) / F;
        ++levels;
    }
    return levels;
}

// Nodes per step of a scan, CHUNK: their loads do not depend on one another,
// so a step costs one latency, not CHUNK of them.  One for a tile in LDS,
// where most walks end at their first or second node; kLpfChunk in global
// memory, where the latency of a dependent load is what a walk costs.
constexpr int kLpfChunk = 16;

// Nodes hi, hi - 1, .. lo of level lv (lo <= hi): the first whose SA minimum is
// below v ends the scan (at = its index, nd = the node); the ones in front of
// it give their LCP minima to m.
template <int CHUNK, class H>
SA_HD bool lpf_scan_down(const H& h, int lv, uint64_t hi, uint64_t lo, uint32_t v, uint32_t& m, uint64_t& at,
                         LpfNode& nd) {
    for (uint64_t c = hi;; c -= CHUNK) {
        const uint64_t left = c - lo + 1;
        int hit = -1;
        // no exit inside: the CHUNK loads are issued together
        SA_LZ_UNROLL
        for (int j = 0; j < CHUNK; ++j) {
            const LpfNode x = h(lv, (uint64_t)j < left ? c - j : c);   // past the run: node c again
            if ((uint64_t)j < left && hit < 0) {
                if (x.sa < v) {
                    hit = j;
                    nd = x;
                } else {
                    m = lz_min32(m, x.lcp);
                }
            }
        }
        if (hit >= 0) {
            at = c - (uint64_t)hit;
            return true;
        }
        if (left <= (uint64_t)CHUNK) return false;
    }
}

// nodes lo, lo + 1, .. hi - 1 of level lv (lo < hi), in that order
template <int CHUNK, class H>
SA_HD bool lpf_scan_up(const H& h, int lv, uint64_t lo, uint64_t hi, uint32_t v, uint32_t& m, uint64_t& at,
                       LpfNode& nd) {
    for (uint64_t c = lo;; c += CHUNK) {
        const uint64_t left = hi - c;
        int hit = -1;
        SA_LZ_UNROLL
        for (int j = 0; j < CHUNK; ++j) {
            const LpfNode x = h(lv, (uint64_t)j < left ? c + j : c);
            if ((uint64_t)j < left && hit < 0) {
                if (x.sa < v) {
                    hit = j;
                    nd = x;
                } else {
                    m = lz_min32(m, x.lcp);
                }
            }
        }
        if (hit >= 0) {
            at = c + (uint64_t)hit;
            return true;
        }
        if (left <= (uint64_t)CHUNK) return false;
    }
}

// The nearest rank below r whose SA entry is below v, over the hierarchy `h`
// (h(level, idx): the node; h.count(level): the level's nodes; h.levels()).
// m comes in as lcp[r] and leaves as min lcp(a + 1 .. r], val = SA[a].  False
// when there is none; m is then the minimum down to rank 0, and a caller
// whose hierarchy is a window goes on from the window's first rank with it.
template <uint32_t F, int CHUNK, class H>
SA_HD bool lpf_walk_left(const H& h, uint64_t r, uint32_t v, uint32_t& m, uint32_t& val) {
    if (r == 0) return false;
    const int levels = h.levels();
    uint64_t idx = r - 1;
    int lv = 0;
    LpfNode nd;
    for (;;) {
        // the last child of its parent: the parent ends where it ends
        while (lv + 1 < levels && idx % F == F - 1) {
            idx /= F;
            ++lv;
        }
        // down to the first child of the same parent (to node 0 at the top)
        const uint64_t lo = lv + 1 < levels ? idx - idx % F : 0;
        if (lpf_scan_down<CHUNK>(h, lv, idx, lo, v, m, idx, nd)) break;
        if (lo == 0) return false;
        idx = lo - 1;
    }
    while (lv > 0) {   // the answer is inside node idx: its last child that holds one
        --lv;
        const uint64_t first = idx * F;
        uint64_t c = first + F - 1;
        if (c >= h.count(lv)) c = h.count(lv) - 1;
        if (!lpf_scan_down<CHUNK>(h, lv, c, first, v, m, idx, nd)) return false;   // a node that does not hold its own minimum
    }
    val = nd.sa;
    return true;
}

// The nearest rank above r whose SA entry is below v.  m comes in as all ones
// (or what a window's walk left) and leaves as min lcp(r + 1 .. b], val =
// SA[b].  False when there is none.
template <uint32_t F, int CHUNK, class H>
SA_HD bool lpf_walk_right(const H& h, uint64_t r, uint32_t v, uint32_t& m, uint32_t& val) {
    const int levels = h.levels();
    uint64_t idx = r + 1;
    int lv = 0;
    if (idx >= h.count(0)) return false;
    LpfNode nd;
    for (;;) {
        // the first child of its parent: the parent starts where it starts
        while (lv + 1 < levels && idx % F == 0) {
            idx /= F;
            ++lv;
        }
        // up to the last child of the same parent (to the last node at the top)
        uint64_t hi = lv + 1 < levels ? idx - idx % F + F : h.count(lv);
        if (hi > h.count(lv)) hi = h.count(lv);
        if (lpf_scan_up<CHUNK>(h, lv, idx, hi, v, m, idx, nd)) break;
        if (hi >= h.count(lv)) return false;
        idx = hi;
    }
    while (lv > 0) {
        --lv;
        const uint64_t first = idx * F;
        uint64_t end = first + F;
        if (end > h.count(lv)) end = h.count(lv);
        if (first >= end || !lpf_scan_up<CHUNK>(h, lv, first, end, v, m, idx, nd)) return false;
    }
    m = lz_min32(m, nd.lcp);   // lcp[b] belongs to the range
    val = nd.sa;
    return true;
}

// LPF and the canonical SRC from the two sides (found, minimum, SA entry)
SA_HD void lpf_combine(bool fa, uint32_t la, uint32_t va, bool fb, uint32_t lb, uint32_t vb, uint32_t& lpf,
                       uint32_t& src) {
    if (!fa) la = 0;
    if (!fb) lb = 0;
    lpf = la > lb ? la : lb;
    src = (la >= lb && la > 0) ? va : (lb > 0 ? vb : kLpfNone);
}

// the phrase that starts at i ends here: in 64 bits, at most n (i < n)
SA_HD uint64_t lz_next(uint64_t i, uint32_t lpf, uint64_t n) {
    const uint64_t x = i + (lpf ? (uint64_t)lpf : 1ull);
    return x < n ? x : n;
}

// One round of pointer jumping inside the tile [base, end): e(i) is on the
// path from i and past i; a value at or past `end` is final.  at(k): the
// current value of tile slot k (any value it held during the round will do).
template <class At>
SA_HD uint32_t lz_jump(uint32_t x, uint64_t base, uint64_t end, const At& at) {
    return (uint64_t)x < end ? at((uint32_t)((uint64_t)x - base)) : x;
}

// first index in [0, c) with cand(k) >= x, else c
template <class Cand>
SA_HD uint64_t lz_cand_index(const Cand& cand, uint64_t c, uint64_t x) {
    uint64_t a = 0, len = c;
    while (len > 0) {
        const uint64_t half = len >> 1;
        if (cand(a + half) < x) {
            a += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return a;
}

// the successor of a candidate whose exit is e: the exit's index, c (the end)
// when the exit is n or is no candidate
template <class Cand>
SA_HD uint64_t lz_cand_succ(const Cand& cand, uint64_t c, uint64_t e, uint64_t n) {
    if (e >= n) return c;
    const uint64_t k = lz_cand_index(cand, c, e);
    return k < c && cand(k) == e ? k : c;
}

// rounds of flag[J[k]] |= flag[k]; J = J o J that flag a path of up to c members
SA_HD int lz_reach_rounds(uint64_t c) {
    int t = 0;
    while (t < 64 && (1ull << t) < c) ++t;
    return t;
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

namespace sa {

static_assert(SA_LPF_NONE == kLpfNone, "sa_hip.h states this");
static_assert(kLzTile == kLzFan * kLzFan && kLzTile == (uint32_t)kTile && kLzFan == (uint32_t)kWave,
              "a tile is two levels; a wavefront reduces one node");
constexpr int kLzPer = (int)(kLzTile / kBlock);   // 16 entries per lane
constexpr int kLzRounds = 12;                     // 2^12 = kLzTile hops
static_assert((1u << kLzRounds) == kLzTile && kLzPer == 16, "one uint16 of path bits per lane");

// the global hierarchy: level 0 is (sa, lcp), level k >= 1 is node[k]
struct LpfLevels {
    const uint32_t* __restrict__ sa;
    const uint32_t* __restrict__ lcp;
    const uint2* node[kLpfMaxLevels];
    uint64_t cnt[kLpfMaxLevels];
    int n_levels;
    __device__ __forceinline__ int levels() const { return n_levels; }
    __device__ __forceinline__ uint64_t count(int lv) const { return cnt[lv]; }
    __device__ __forceinline__ LpfNode operator()(int lv, uint64_t i) const {
        if (lv == 0) return LpfNode{sa[i], lcp[i]};
        const uint2 x = node[lv][i];
        return LpfNode{x.x, x.y};
    }
};

// a tile in LDS: c0 (sa, lcp) pairs, c1 level-1 nodes, one level-2 node
struct LpfLocal {
    const uint2* s_l0;
    const uint2* s_l1;
    const uint2* s_l2;
    uint32_t c0, c1;
    __device__ __forceinline__ int levels() const { return 3; }
    __device__ __forceinline__ uint64_t count(int lv) const { return lv == 0 ? c0 : lv == 1 ? c1 : 1u; }
    __device__ __forceinline__ LpfNode operator()(int lv, uint64_t i) const {
        const uint2 x = lv == 0 ? s_l0[i] : lv == 1 ? s_l1[i] : s_l2[0];
        return LpfNode{x.x, x.y};
    }
};

// Tile `tile` of SA and LCP into LDS (what lies past n reads as all ones, the
// minimum's identity), its level-1 nodes into s_l1 and its level-2 node into
// s_l2[0].  Ends with a barrier.
__device__ __forceinline__ void lpf_load_tile(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ lcp,
                                              uint64_t n, uint64_t tile, uint2* s_l0, uint2* s_l1, uint2* s_l2) {
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    const uint64_t base = tile * kLzTile;
#pragma unroll
    for (int j = 0; j < kLzPer; ++j) {
        const uint32_t i = j * kBlock + tid;
        const bool in = base + i < n;
        s_l0[i] = in ? make_uint2(sa[base + i], lcp[base + i]) : make_uint2(~0u, ~0u);
    }
    __syncthreads();
    constexpr uint32_t per_wave = kLzFan / kWaves;   // 16 nodes per wavefront
    for (uint32_t k = 0; k < per_wave; ++k) {
        const uint32_t node = wave * per_wave + k;
        const uint2 e = s_l0[node * kLzFan + lane];
        uint32_t x = e.x, y = e.y;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            x = lz_min32(x, (uint32_t)__shfl_xor((int)x, o, kWave));
            y = lz_min32(y, (uint32_t)__shfl_xor((int)y, o, kWave));
        }
        if (lane == 0) s_l1[node] = make_uint2(x, y);
    }
    __syncthreads();
    if (wave == 0) {
        uint32_t x = s_l1[lane].x, y = s_l1[lane].y;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            x = lz_min32(x, (uint32_t)__shfl_xor((int)x, o, kWave));
            y = lz_min32(y, (uint32_t)__shfl_xor((int)y, o, kWave));
        }
        if (lane == 0) s_l2[0] = make_uint2(x, y);
    }
    __syncthreads();
}

// c1 = the nodes of level 1 (ceil(n / 64)); l2 is NULL when level 1 is the top
__global__ __launch_bounds__(kBlock) void k_lpf_minima(const uint32_t* __restrict__ sa,
                                                       const uint32_t* __restrict__ lcp, uint64_t n, uint64_t c1,
                                                       uint2* __restrict__ l1, uint2* __restrict__ l2) {
    __shared__ uint2 s_l0[kLzTile], s_l1[kLzFan], s_l2[1];
    const uint64_t tile = blockIdx.x;
    lpf_load_tile(sa, lcp, n, tile, s_l0, s_l1, s_l2);
    const uint64_t g = tile * kLzFan + threadIdx.x;
    if (threadIdx.x < kLzFan && g < c1) l1[g] = s_l1[threadIdx.x];
    if (threadIdx.x == 0 && l2) l2[tile] = s_l2[0];
}

// out[p] = the minima of in[p * 64 .. p * 64 + 64) (cut at cin)
__global__ __launch_bounds__(kBlock) void k_lpf_reduce(const uint2* __restrict__ in, uint64_t cin,
                                                       uint2* __restrict__ out, uint64_t cout) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= cout) return;
    uint32_t x = ~0u, y = ~0u;
    const uint64_t e = std::min<uint64_t>(p * kLzFan + kLzFan, cin);
    for (uint64_t i = p * kLzFan; i < e; ++i) {
        const uint2 v = in[i];
        x = lz_min32(x, v.x);
        y = lz_min32(y, v.y);
    }
    out[p] = make_uint2(x, y);
}

__global__ __launch_bounds__(kBlock) void k_lpf_resolve(LpfLevels g, uint64_t n, uint32_t* __restrict__ lpf,
                                                        uint32_t* __restrict__ src) {
    __shared__ uint2 s_l0[kLzTile], s_l1[kLzFan], s_l2[1];
    const uint64_t tile = blockIdx.x, base = tile * kLzTile;
    lpf_load_tile(g.sa, g.lcp, n, tile, s_l0, s_l1, s_l2);
    LpfLocal loc;
    loc.s_l0 = s_l0;
    loc.s_l1 = s_l1;
    loc.s_l2 = s_l2;
    loc.c0 = (uint32_t)std::min<uint64_t>(kLzTile, n - base);
    loc.c1 = (loc.c0 + kLzFan - 1) / kLzFan;
    for (int j = 0; j < kLzPer; ++j) {
        const uint32_t i = j * kBlock + threadIdx.x;
        if (i >= loc.c0) break;
        const uint32_t v = s_l0[i].x;
        uint32_t la = s_l0[i].y, va = 0, lb = ~0u, vb = 0;
        bool fa = lpf_walk_left<kLzFan, 1>(loc, i, v, la, va);
        if (!fa) fa = lpf_walk_left<kLzFan, kLpfChunk>(g, base, v, la, va);   // from the tile's first rank
        bool fb = lpf_walk_right<kLzFan, 1>(loc, i, v, lb, vb);
        if (!fb) fb = lpf_walk_right<kLzFan, kLpfChunk>(g, base + loc.c0 - 1, v, lb, vb);   // from its last
        uint32_t l, s;
        lpf_combine(fa, la, va, fb, lb, vb, l, s);
        const uint64_t p = std::min<uint64_t>(v, n - 1);   // an SA entry >= n is clamped
        lpf[p] = l;
        src[p] = s;
    }
}

// exit[i] and the marks of the candidates (mask is zero on entry)
__global__ __launch_bounds__(kBlock) void k_lz_exits(const uint32_t* __restrict__ lpf, uint64_t n,
                                                     uint32_t* __restrict__ exit, uint8_t* __restrict__ mask) {
    __shared__ uint32_t s_e[kLzTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kLzTile;
    const uint64_t end = std::min<uint64_t>(base + kLzTile, n);
#pragma unroll
    for (int j = 0; j < kLzPer; ++j) {
        const uint32_t i = j * kBlock + tid;
        s_e[i] = base + i < n ? (uint32_t)lz_next(base + i, lpf[base + i], n) : (uint32_t)n;
    }
    __syncthreads();
    // in place: a slot read while its owner writes it holds its old or its
    // new value, and both are on the path and past the reader's
    for (int round = 0; round < kLzRounds; ++round) {
#pragma unroll
        for (int j = 0; j < kLzPer; ++j) {
            const uint32_t i = j * kBlock + tid;
            s_e[i] = lz_jump(s_e[i], base, end, [&](uint32_t k) { return s_e[k]; });
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < kLzPer; ++j) {
        const uint32_t i = j * kBlock + tid;
        if (base + i >= n) continue;
        const uint32_t e = s_e[i];
        exit[base + i] = e;
        if (e < n && (i == 0 || s_e[i - 1] != e)) mask[e] = 1;
    }
    if (base == 0 && tid == 0) mask[0] = 1;
}

struct LzCand {
    const int64_t* __restrict__ p;
    __device__ __forceinline__ uint64_t operator()(uint64_t k) const { return (uint64_t)p[k]; }
};

// J[k] = the index of candidate k's exit (c: the end), J[c] = c; flag[0] = 1
__global__ __launch_bounds__(kBlock) void k_lz_succ(const int64_t* __restrict__ cand, uint64_t c,
                                                    const uint32_t* __restrict__ exit, uint64_t n,
                                                    uint32_t* __restrict__ J, uint32_t* __restrict__ flag) {
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k <= c; k += (uint64_t)gridDim.x * kBlock) {
        uint64_t j = c;
        if (k < c) {
            const uint64_t p = std::min<uint64_t>((uint64_t)cand[k], n - 1);
            j = lz_cand_succ(LzCand{cand}, c, exit[p], n);
        }
        J[k] = (uint32_t)j;
        flag[k] = k == 0 ? 1u : 0u;
    }
}

// one round; a flag set during the round may be seen early: it is then one
// the next round would set
__global__ __launch_bounds__(kBlock) void k_lz_reach(const uint32_t* __restrict__ Jin, uint32_t* __restrict__ Jout,
                                                     uint32_t* flag, uint64_t c) {
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k <= c; k += (uint64_t)gridDim.x * kBlock) {
        const uint64_t j = std::min<uint64_t>(Jin[k], c);
        if (j < c && flag[k]) flag[j] = 1u;
        Jout[k] = Jin[j];
    }
}

// entry[t] = the flagged candidate inside tile t (all ones on entry: none)
__global__ __launch_bounds__(kBlock) void k_lz_entry(const int64_t* __restrict__ cand, const uint32_t* __restrict__ flag,
                                                     uint64_t c, uint64_t n, uint32_t* __restrict__ entry) {
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < c; k += (uint64_t)gridDim.x * kBlock) {
        const uint64_t p = (uint64_t)cand[k];
        if (flag[k] && p < n) entry[p / kLzTile] = (uint32_t)p;
    }
}

// bits[t * kBlock + lane of the workgroup]: bit j = position t * kLzTile + 16 *
// lane + j starts a phrase; tcnt[t] = the tile's phrases
__global__ __launch_bounds__(kBlock) void k_lz_mark(const uint32_t* __restrict__ lpf, uint64_t n,
                                                    const uint32_t* __restrict__ entry, uint16_t* __restrict__ bits,
                                                    int64_t* __restrict__ tcnt) {
    __shared__ uint16_t s_j[2][kLzTile];   // the next member's slot; kLzTile: outside the tile
    __shared__ uint8_t s_f[kLzTile];
    __shared__ uint32_t s_w[kWaves];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kLzTile;
    const uint64_t end = std::min<uint64_t>(base + kLzTile, n);
    const uint64_t e = entry[blockIdx.x];
    if (e < base || e >= end) {   // uniform: the parse jumps over this tile
        if (tid == 0) tcnt[blockIdx.x] = 0;
        return;
    }
#pragma unroll
    for (int j = 0; j < kLzPer; ++j) {
        const uint32_t i = j * kBlock + tid;
        uint32_t x = kLzTile;
        if (base + i < n) {
            const uint64_t nx = lz_next(base + i, lpf[base + i], n);
            if (nx < end) x = (uint32_t)(nx - base);
        }
        s_j[0][i] = (uint16_t)x;
        s_f[i] = base + i == e ? 1 : 0;
    }
    __syncthreads();
    for (int round = 0; round < kLzRounds; ++round) {
        const uint16_t* cur = s_j[round & 1];
        uint16_t* nxt = s_j[(round + 1) & 1];
#pragma unroll
        for (int j = 0; j < kLzPer; ++j) {
            const uint32_t i = j * kBlock + tid;
            const uint32_t x = cur[i];
            if (x < kLzTile) {
                if (s_f[i]) s_f[x] = 1;
                nxt[i] = cur[x];
            } else {
                nxt[i] = (uint16_t)kLzTile;
            }
        }
        __syncthreads();
    }
    uint32_t b = 0;
#pragma unroll
    for (int j = 0; j < kLzPer; ++j) b |= s_f[kLzPer * tid + j] ? 1u << j : 0u;
    uint32_t sum;
    (void)mem_block_excl((uint32_t)__popc(b), s_w, sum);
    bits[(uint64_t)blockIdx.x * kBlock + tid] = (uint16_t)b;
    if (tid == 0) tcnt[blockIdx.x] = (int64_t)sum;
}

// tbase: the inclusive sums of the tile counts; nothing is written when z
// exceeds out_cap
__global__ __launch_bounds__(kBlock) void k_lz_emit(const uint32_t* __restrict__ lpf, const uint32_t* __restrict__ src,
                                                    uint64_t n, const uint16_t* __restrict__ bits,
                                                    const int64_t* __restrict__ tbase, uint64_t out_cap,
                                                    uint32_t* __restrict__ pos, uint32_t* __restrict__ len,
                                                    uint32_t* __restrict__ fsrc) {
    __shared__ uint32_t s_w[kWaves];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x;
    const uint64_t z = (uint64_t)tbase[gridDim.x - 1];
    const uint64_t first = t ? (uint64_t)tbase[t - 1] : 0;
    if (z > out_cap || (uint64_t)tbase[t] == first) return;   // uniform; an empty tile's bits were never written
    uint32_t b = bits[t * kBlock + tid];
    uint32_t sum;
    uint64_t o = first + mem_block_excl((uint32_t)__popc(b), s_w, sum);
    while (b) {
        const int j = __builtin_ctz(b);
        b &= b - 1u;
        const uint64_t i = t * kLzTile + (uint64_t)kLzPer * tid + j;
        if (i >= n || o >= z) break;
        const uint32_t l = lpf[i];
        pos[o] = (uint32_t)i;
        len[o] = (uint32_t)(lz_next(i, l, n) - i);
        fsrc[o] = l ? src[i] : kLpfNone;
        ++o;
    }
}

// the checks of sa_lpf_device, all before any HIP call
static int lpf_check_args(const sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                          const uint32_t* d_lcp, const uint32_t* d_lpf, const uint32_t* d_src) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (n == 0) return SA_OK;
    if (!d_sa) return set_err(SA_E_INVALID, "d_sa is NULL");
    if (!d_lpf) return set_err(SA_E_INVALID, "d_lpf is NULL");
    if (!d_src) return set_err(SA_E_INVALID, "d_src is NULL");
    if (!d_text && !d_lcp) return set_err(SA_E_INVALID, "d_text and d_lcp are both NULL");
    if ((uintptr_t)d_lpf & 3u) return set_err(SA_E_INVALID, "d_lpf is not 4-byte aligned");
    if ((uintptr_t)d_src & 3u) return set_err(SA_E_INVALID, "d_src is not 4-byte aligned");
    SA_TRY(check_no_alias({d_lpf, d_src}, {d_text, d_sa, d_lcp}));
    return check_distinct({d_lpf, d_src});
}

static int lpf_device(sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lcp,
                      uint32_t* d_lpf, uint32_t* d_src, hipStream_t s) {
    SA_TRY(lpf_check_args(c, d_text, n, d_sa, d_lcp, d_lpf, d_src));
    if (n == 0) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    if (n == 1) {
        SA_HIP(hipMemsetAsync(d_lpf, 0, 4, s));
        SA_HIP(hipMemsetAsync(d_src, 0xFF, 4, s));
        return SA_OK;
    }
    LocBuf own_lcp;
    if (!d_lcp) {
        SA_TRY(own_lcp.alloc(align_up(n, 64) * 4, s));
        SA_TRY(lcp_device(c, d_text, n, d_sa, (uint32_t*)own_lcp.p, nullptr, s));
        d_lcp = (const uint32_t*)own_lcp.p;
    }
    LpfLevels g;
    g.sa = d_sa;
    g.lcp = d_lcp;
    g.n_levels = lpf_level_counts<kLzFan>(n, g.cnt);
    uint64_t nodes = 0;
    for (int lv = 1; lv < g.n_levels; ++lv) nodes += g.cnt[lv];
    LocBuf hier;
    SA_TRY(hier.alloc(nodes * 8, s));
    {
        uint2* p = (uint2*)hier.p;
        for (int lv = 0; lv < kLpfMaxLevels; ++lv) {
            g.node[lv] = lv >= 1 && lv < g.n_levels ? p : nullptr;
            if (lv >= 1 && lv < g.n_levels) p += g.cnt[lv];
            if (lv >= g.n_levels) g.cnt[lv] = 0;
        }
    }
    const uint64_t tiles = (n + kLzTile - 1) / kLzTile;   // <= 2^20
    hipLaunchKernelGGL(k_lpf_minima, dim3((uint32_t)tiles), dim3(kBlock), 0, s, d_sa, d_lcp, n, g.cnt[1],
                       const_cast<uint2*>(g.node[1]), g.n_levels > 2 ? const_cast<uint2*>(g.node[2]) : nullptr);
    for (int lv = 3; lv < g.n_levels; ++lv)
        hipLaunchKernelGGL(k_lpf_reduce, dim3((uint32_t)((g.cnt[lv] + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           g.node[lv - 1], g.cnt[lv - 1], const_cast<uint2*>(g.node[lv]), g.cnt[lv]);
    hipLaunchKernelGGL(k_lpf_resolve, dim3((uint32_t)tiles), dim3(kBlock), 0, s, g, n, d_lpf, d_src);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// the checks of sa_lz77_device, all before any HIP call
static int lz77_check_args(const sa_context* c, uint64_t n, const uint32_t* d_lpf, const uint32_t* d_src,
                           const uint32_t* d_pos, const uint32_t* d_len, const uint32_t* d_fsrc, const uint64_t* z) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!z) return set_err(SA_E_INVALID, "z is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    const int given = (d_pos ? 1 : 0) + (d_len ? 1 : 0) + (d_fsrc ? 1 : 0);
    if (given != 0 && given != 3) return set_err(SA_E_INVALID, "d_pos, d_len and d_fsrc: all or none");
    if (n == 0) return SA_OK;
    if (!d_lpf) return set_err(SA_E_INVALID, "d_lpf is NULL");
    if (!d_src) return set_err(SA_E_INVALID, "d_src is NULL");
    if (given) {
        if (((uintptr_t)d_pos | (uintptr_t)d_len | (uintptr_t)d_fsrc) & 3u)
            return set_err(SA_E_INVALID, "an output is not 4-byte aligned");
        SA_TRY(check_no_alias({d_pos, d_len, d_fsrc}, {d_lpf, d_src}));
        SA_TRY(check_distinct({d_pos, d_len, d_fsrc}));
    }
    return SA_OK;
}

// Host waits: the candidate count, the candidate list (sa_select_u8_device's
// two calls), z.
static int lz77_device(sa_context* c, uint64_t n, const uint32_t* d_lpf, const uint32_t* d_src, uint32_t* d_pos,
                       uint32_t* d_len, uint32_t* d_fsrc, uint64_t out_cap, uint64_t* z, hipStream_t s) {
    SA_TRY(lz77_check_args(c, n, d_lpf, d_src, d_pos, d_len, d_fsrc, z));
    *z = 0;
    if (n == 0) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    const uint64_t tiles = (n + kLzTile - 1) / kLzTile;
    // exit (n) | mask (n bytes) | entry (tiles) | path bits (tiles * 256 * 2) | tile counts (tiles)
    const uint64_t b_exit = align_up(n, 64) * 4, b_mask = align_up(n, 256), b_entry = align_up(tiles, 64) * 4,
                   b_bits = tiles * kBlock * 2;
    LocBuf tmp;
    SA_TRY(tmp.alloc(b_exit + b_mask + b_entry + b_bits + tiles * 8, s));
    uint32_t* d_exit = (uint32_t*)tmp.p;
    uint8_t* d_mask = (uint8_t*)tmp.p + b_exit;
    uint32_t* d_entry = (uint32_t*)(d_mask + b_mask);
    uint16_t* d_bits = (uint16_t*)((uint8_t*)d_entry + b_entry);
    int64_t* d_tcnt = (int64_t*)((uint8_t*)d_bits + b_bits);
    SA_HIP(hipMemsetAsync(d_mask, 0, b_mask, s));
    SA_HIP(hipMemsetAsync(d_entry, 0xFF, b_entry, s));
    hipLaunchKernelGGL(k_lz_exits, dim3((uint32_t)tiles), dim3(kBlock), 0, s, d_lpf, n, d_exit, d_mask);
    SA_HIP(hipGetLastError());
    uint64_t cands = 0, got = 0;
    SA_TRY(sa_select_u8_device(d_mask, n, nullptr, &cands, s));
    if (cands == 0 || cands > n) return set_err(SA_E_INTERNAL, "lz77: %llu candidates", (unsigned long long)cands);
    {
        // candidates (c int64) | J, J' and flags (c + 1 uint32 each)
        const uint64_t w = align_up(cands + 1, 64);
        LocBuf cb;
        SA_TRY(cb.alloc(cands * 8 + 3 * w * 4, s));
        int64_t* d_cand = (int64_t*)cb.p;
        uint32_t* d_j[2] = {(uint32_t*)(d_cand + cands), (uint32_t*)(d_cand + cands) + w};
        uint32_t* d_flag = d_j[1] + w;
        SA_TRY(sa_select_u8_device(d_mask, n, d_cand, &got, s));
        if (got != cands)
            return set_err(SA_E_INTERNAL, "lz77: %llu candidates after %llu were counted", (unsigned long long)got,
                           (unsigned long long)cands);
        const uint32_t grid = (uint32_t)std::min<uint64_t>((cands + kBlock) / kBlock, (uint64_t)c->cus * 8);
        hipLaunchKernelGGL(k_lz_succ, dim3(grid), dim3(kBlock), 0, s, (const int64_t*)d_cand, cands,
                           (const uint32_t*)d_exit, n, d_j[0], d_flag);
        const int rounds = lz_reach_rounds(cands);
        for (int t = 0; t < rounds; ++t)
            hipLaunchKernelGGL(k_lz_reach, dim3(grid), dim3(kBlock), 0, s, (const uint32_t*)d_j[t & 1], d_j[(t + 1) & 1],
                               d_flag, cands);
        hipLaunchKernelGGL(k_lz_entry, dim3(grid), dim3(kBlock), 0, s, (const int64_t*)d_cand, (const uint32_t*)d_flag,
                           cands, n, d_entry);
        SA_HIP(hipGetLastError());
        SA_TRACE("lz77: n %llu candidates %llu (%.2f per tile), %d rounds", (unsigned long long)n,
                 (unsigned long long)cands, (double)cands / (double)tiles, rounds);
    }
    hipLaunchKernelGGL(k_lz_mark, dim3((uint32_t)tiles), dim3(kBlock), 0, s, d_lpf, n, (const uint32_t*)d_entry, d_bits,
                       d_tcnt);
    SA_HIP(hipGetLastError());
    SA_TRY(scan_i64<ScanSum>(d_tcnt, tiles, s));
    if (d_pos) {
        hipLaunchKernelGGL(k_lz_emit, dim3((uint32_t)tiles), dim3(kBlock), 0, s, d_lpf, d_src, n,
                           (const uint16_t*)d_bits, (const int64_t*)d_tcnt, out_cap, d_pos, d_len, d_fsrc);
        SA_HIP(hipGetLastError());
    }
    uint64_t* h = host_u64<kHwLz, 1>(c);
    SA_HIP(hipMemcpyAsync(h, d_tcnt + (tiles - 1), 8, hipMemcpyDeviceToHost, s));
    SA_HIP(host_sync(s));
    *z = h[0];
    return SA_OK;
}

// what sa_lpf and sa_lz77 check alike, and the text and SA on the device with
// LPF and SRC computed (the SA is checked first: PHI scatters through it)
struct LzHost {
    DevBuf text, sa, lpf, src;
    sa_context* c = nullptr;
};
static int lz_host_args(const uint8_t* text, uint64_t n, const void* sa, int sa_width) {
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (n && !text) return set_err(SA_E_INVALID, "text is NULL");
    if (n && !sa) return set_err(SA_E_INVALID, "sa is NULL");
    return SA_OK;
}
static int lz_host_lpf(const uint8_t* text, uint64_t n, const void* src32, LzHost& h) {
    SA_TRY(global_ctx(n, &h.c));
    SA_TRY(h.text.alloc(align_up(n, 256)));
    SA_TRY(h.sa.alloc(align_up(n, 64) * 4));
    SA_TRY(h.lpf.alloc(align_up(n, 64) * 4));
    SA_TRY(h.src.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{h.text.p, text, n}, {h.sa.p, src32, n * 4}}));
    const int valid = check_device(h.c, h.text.as<uint8_t>(), n, h.sa.as<uint32_t>(), nullptr);
    if (valid == 0) return set_err(SA_E_INVALID, "not a valid suffix array of the text");
    if (valid != 1) return valid;
    return lpf_device(h.c, h.text.as<uint8_t>(), n, h.sa.as<uint32_t>(), nullptr, h.lpf.as<uint32_t>(),
                      h.src.as<uint32_t>(), nullptr);
}
// width 8: "none" is all ones
static void lz_widen_none(void* out, uint64_t count, int width) {
    if (width != 8 || !out) return;
    int64_t* o = (int64_t*)out;
    for (uint64_t i = 0; i < count; ++i)
        if (o[i] == (int64_t)kLpfNone) o[i] = -1;
}

static int lpf_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* lpf_out, void* src_out) {
    SA_TRY(lz_host_args(text, n, sa, sa_width));
    if (n && !lpf_out) return set_err(SA_E_INVALID, "lpf_out is NULL");
    if (n && !src_out) return set_err(SA_E_INVALID, "src_out is NULL");
    if (n && (lpf_out == src_out || lpf_out == (const void*)text || lpf_out == sa || src_out == (const void*)text ||
              src_out == sa))
        return set_err(SA_E_INVALID, "an output aliases an input or the other output");
    if (n == 0) return SA_OK;
    std::vector<uint32_t> narrow;
    const void* src32 = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src32));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    LzHost h;
    SA_TRY(lz_host_lpf(text, n, src32, h));
    SA_TRY(copy_d2h(lpf_out, h.lpf.as<uint32_t>(), n, sa_width, nullptr));
    SA_TRY(copy_d2h(src_out, h.src.as<uint32_t>(), n, sa_width, nullptr));
    lz_widen_none(src_out, n, sa_width);
    return SA_OK;
}

// LPF on the device once, the sizing parse, then the writing parse into
// buffers made for z phrases: only z crosses to the host in between
static int lz77_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* pos_out, void* len_out,
                     void* src_out, uint64_t out_cap, uint64_t* z) {
    SA_TRY(lz_host_args(text, n, sa, sa_width));
    if (!z) return set_err(SA_E_INVALID, "z is NULL");
    const int given = (pos_out ? 1 : 0) + (len_out ? 1 : 0) + (src_out ? 1 : 0);
    if (given != 0 && given != 3) return set_err(SA_E_INVALID, "pos_out, len_out and src_out: all or none");
    SA_TRY(check_distinct({pos_out, len_out, src_out}));
    SA_TRY(check_no_alias({pos_out, len_out, src_out}, {text, sa}));
    *z = 0;
    if (n == 0) return SA_OK;
    std::vector<uint32_t> narrow;
    const void* src32 = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src32));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    LzHost h;
    SA_TRY(lz_host_lpf(text, n, src32, h));
    SA_TRY(lz77_device(h.c, n, h.lpf.as<uint32_t>(), h.src.as<uint32_t>(), nullptr, nullptr, nullptr, 0, z, nullptr));
    if (!given || *z > out_cap) return SA_OK;
    DevBuf d_pos, d_len, d_fsrc;
    SA_TRY(d_pos.alloc(align_up(*z, 64) * 4));
    SA_TRY(d_len.alloc(align_up(*z, 64) * 4));
    SA_TRY(d_fsrc.alloc(align_up(*z, 64) * 4));
    uint64_t got = 0;
    SA_TRY(lz77_device(h.c, n, h.lpf.as<uint32_t>(), h.src.as<uint32_t>(), d_pos.as<uint32_t>(), d_len.as<uint32_t>(),
                       d_fsrc.as<uint32_t>(), *z, &got, nullptr));
    if (got != *z)
        return set_err(SA_E_INTERNAL, "lz77: %llu phrases after a sizing call that counted %llu",
                       (unsigned long long)got, (unsigned long long)*z);
    SA_TRY(copy_d2h(pos_out, d_pos.as<uint32_t>(), *z, sa_width, nullptr));
    SA_TRY(copy_d2h(len_out, d_len.as<uint32_t>(), *z, sa_width, nullptr));
    SA_TRY(copy_d2h(src_out, d_fsrc.as<uint32_t>(), *z, sa_width, nullptr));
    lz_widen_none(src_out, *z, sa_width);
    return SA_OK;
}

}  // namespace sa

extern "C" {

int sa_lpf_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lcp,
                  uint32_t* d_lpf, uint32_t* d_src, void* stream) {
    return sa::lpf_device(ctx, d_text, n, d_sa, d_lcp, d_lpf, d_src, (hipStream_t)stream);
}

int sa_lz77_device(sa_context* ctx, uint64_t n, const uint32_t* d_lpf, const uint32_t* d_src, uint32_t* d_pos,
                   uint32_t* d_len, uint32_t* d_fsrc, uint64_t out_cap, uint64_t* z, void* stream) {
    return sa::lz77_device(ctx, n, d_lpf, d_src, d_pos, d_len, d_fsrc, out_cap, z, (hipStream_t)stream);
}

int sa_lpf(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* lpf_out, void* src_out) {
    return sa::lpf_host(text, n, sa, sa_width, lpf_out, src_out);
}

int sa_lz77(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* pos_out, void* len_out, void* src_out,
            uint64_t out_cap, uint64_t* z) {
    return sa::lz77_host(text, n, sa, sa_width, pos_out, len_out, src_out, out_cap, z);
}

}  // extern "C"

#endif   // __HIPCC__
