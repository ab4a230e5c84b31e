// sa_mem.h -- maximal exact matches of a query against the text (sa_mems /
// sa_mems_device of include/sa_hip.h).
//
// A MEM is (i, p, l): Q[i .. i + l) == T[p .. p + l), l >= L = min_len, not
// extendable to the right (i + l == m, p + l == n, or the next bytes differ)
// nor to the left (i == 0, p == 0, or the bytes in front differ).  Output:
// every MEM once, by (i, p) ascending, in CSR form over the query positions.
//
// The seed search and the hit lists exist already; this header is the part
// in between.
//   seeds        match_stats_device with max_len = L: position i is a seed
//                position when len[i] == L, and [lo, hi) is then every
//                occurrence of Q[i .. i + L).
//   k_mem_seeds  empties the interval of a position that is no seed or whose
//                seed occurs more than max_occ times, and counts candidates
//                (the hits that stay) and skipped positions into two words.
//                The host reads them (the first wait) and applies
//                max_candidates.
//   candidates   locate_device on those intervals, sorted: cand[coff[i] ..
//                coff[i + 1]) are position i's hits, so the list is in (i, p)
//                order.
//   the MEM list is a stable compaction of the candidate list.  Candidate
//                (i, p) survives iff it is left-maximal, and each survivor
//                gives one MEM: a MEM of at least L bytes starts with a seed
//                hit at its own (i, p), which is left-maximal by definition,
//                and a left-maximal hit extends to the right in one way.
//   k_mem_flag   a persistent grid over tiles of kMemTile candidates: the
//                positions of a tile's candidates from coff (two lower bounds
//                per tile, the segment starts marked in LDS and spread by a
//                max-scan, as locate_tile's), one byte gather T[p - 1]
//                against Q[i - 1], the survivors per tile counted and the
//                flags kept, one byte per lane (8 candidates).
//   scan         scan_i64<ScanSum> over the tile counts.
//   k_mem_emit   per tile: ranks of the survivors (popcount inside the lane,
//                a shuffle scan inside the wavefront, LDS across wavefronts),
//                off[i] = the survivors in front of coff[i] for the positions
//                whose list starts in the tile (the last tile takes those at
//                the very end and off[m]), and when the total fits the
//                outputs: l = the bytes Q from i and T from p share, from
//                byte L on, cut at both ends; tpos and len at tile base +
//                rank.  The kernel reads the total on the device, so it is
//                launched before the host knows it; the host reads the total
//                in the last wait.
//   extension    by lane over 8-byte words.  In auto mode a lane gives up
//                after kMemLaneBytes and appends its candidate to an LDS list
//                (one entry per slot of the tile: it cannot overflow); when
//                the tile's lanes are done the wavefronts take the listed
//                candidates one each, 512 bytes a step, first mismatch by
//                ballot.  SA_MEM_LANE / SA_MEM_WAVE force one path.
//
// The seed rule, the left check, the extension and the clamp compile on the
// host: tests/cpp/mem_check.cpp checks them against brute force.
// Measurements and the resource report: DESIGN.md section 14.
// The HIP part needs sa_match.h, sa_locate.h and sa_build.hip's scan_i64
// before it.
#pragma once
#include <stdint.h>

#include "sa_search.h"   // SA_HD

namespace sa {

// a lane's extension in auto mode before it hands over to a wavefront
// (bytes past the seed; a multiple of 8)
constexpr uint64_t kMemLaneBytes = 512;

// candidates of position i: the occurrences of its seed, 0 when the longest
// match under the cap L is shorter than L (no seed), when the interval breaks
// lo <= hi <= n, or when the seed occurs more than max_occ times (0 = no
// filter); the last case alone sets skipped
SA_HD uint32_t mem_seed_count(uint64_t len, uint64_t lo, uint64_t hi, uint64_t n, uint64_t L, uint64_t max_occ,
                              bool& skipped) {
    skipped = false;
    if (len < L || lo > hi || hi > n) return 0u;
    const uint64_t c = hi - lo;
    if (max_occ && c > max_occ) {
        skipped = true;
        return 0u;
    }
    return (uint32_t)c;   // n <= 2^32 - 1
}

// a text position as the kernels use it: an SA entry >= n reads as n - 1 (n >= 1)
SA_HD uint64_t mem_clamp_pos(uint64_t p, uint64_t n) { return p < n ? p : n - 1; }

// (i, p) cannot be extended to the left; q_byte = Q[i - 1] and t_byte =
// T[p - 1] are looked at only when both exist
SA_HD bool mem_left_maximal(uint64_t i, uint64_t p, uint8_t q_byte, uint8_t t_byte) {
    return i == 0 || p == 0 || q_byte != t_byte;
}

// The bytes Q from i and T from p share, given that the first `start` are
// shared: at most min(n - p, m - i).  text_word(x) / query_word(x): the
// little-endian 8 bytes at position x of the text / the query, zero at or past
// the end (load8).  At most max_words words are compared; done = false when
// they ran out before a mismatch or an end, and the result is then the bytes
// known to be shared.  No access is at or past lim = min(n - p, m - i) bytes
// from p or i.
template <class TextWord, class QueryWord>
SA_HD uint64_t mem_extend_steps(uint64_t i, uint64_t p, uint64_t start, uint64_t n, uint64_t m,
                                const TextWord& text_word, const QueryWord& query_word, uint64_t max_words,
                                bool& done) {
    const uint64_t tl = p < n ? n - p : 0, ql = i < m ? m - i : 0;
    const uint64_t lim = tl < ql ? tl : ql;
    done = true;
    for (uint64_t off = start; off < lim; off += 8) {
        if (max_words == 0) {
            done = false;
            return off;
        }
        --max_words;
        const uint64_t d = text_word(p + off) ^ query_word(i + off);
        if (d) {
            const uint64_t j = off + (uint64_t)(__builtin_ctzll(d) >> 3);
            return j < lim ? j : lim;
        }
    }
    return lim;
}

template <class TextWord, class QueryWord>
SA_HD uint64_t mem_extend(uint64_t i, uint64_t p, uint64_t start, uint64_t n, uint64_t m, const TextWord& text_word,
                          const QueryWord& query_word) {
    bool done;
    return mem_extend_steps(i, p, start, n, m, text_word, query_word, ~0ull, done);
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

namespace sa {

static_assert(SA_MEM_INFO == 3 && SA_MEM_TOO_MANY == 1 && SA_MEM_LANE == 1u && SA_MEM_WAVE == 2u,
              "sa_hip.h states these");
static_assert(kMemLaneBytes % 8 == 0, "whole words");

constexpr int kMemPer = 8;                               // candidates per lane
constexpr uint32_t kMemTile = kMemPer * kBlock;          // candidates per tile
constexpr uint32_t kMemGridPerCu = 4;                    // workgroups per CU of the persistent grids
constexpr int kMemHostWord = 3080;                       // host_words: candidates, skipped | total (8 bytes each)
static_assert(kMemTile == 2048, "16-bit slots, one flag byte per lane");

// exclusive prefix of v over the workgroup's lanes, and the workgroup's sum
__device__ __forceinline__ uint32_t mem_block_excl(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const uint32_t lane = lane_id(), wave = threadIdx.x / kWave;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o, kWave);
        if ((int)lane >= o) incl += y;
    }
    if (lane == kWave - 1) s_w[wave] = incl;
    __syncthreads();
    uint32_t c = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kWaves; ++w) {
        const uint32_t x = s_w[w];
        if (w < wave) c += x;
        total += x;
    }
    __syncthreads();   // s_w may be written again
    return c + incl - v;
}

// Tile t of the candidate list: candidates [s, s + cnt); the positions whose
// list starts inside it are [q_lo, q_hi) (coff(q) in [s, s + cnt)), the empty
// ones among them included.
struct MemTile {
    uint64_t s, q_lo, q_hi;
    uint32_t cnt;
};

// The query position of each of the tile's candidates: s_pos[slot] for all
// kMemTile slots (what lies past cnt repeats the last position), and the
// calling lane's own kMemPer contiguous slots in pos.  s_q: 2 words, s_w:
// kWaves words.  Ends with a barrier.
__device__ __forceinline__ MemTile mem_tile_positions(const uint64_t* __restrict__ coff, uint64_t m, uint64_t t,
                                                      uint64_t total, uint32_t* s_pos, uint32_t* s_w, uint64_t* s_q,
                                                      uint32_t (&pos)[kMemPer]) {
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    MemTile r;
    r.s = t * kMemTile;
    r.cnt = (uint32_t)std::min<uint64_t>(kMemTile, total - r.s);
    if (tid == 0) {
        // coff has m + 1 entries and coff[m] = total >= s + cnt: both bounds are at most m
        const uint64_t a = locate_lower_bound(LocOff{coff}, 0, m + 1, r.s);
        s_q[0] = a;
        s_q[1] = locate_lower_bound(LocOff{coff}, a, m + 1, r.s + r.cnt);
    }
    {
        uint4* mine = reinterpret_cast<uint4*>(s_pos + kMemPer * tid);
        mine[0] = make_uint4(0u, 0u, 0u, 0u);
        mine[1] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    r.q_lo = s_q[0];
    r.q_hi = s_q[1];
    // a non-empty position marks the slot of its first candidate with q + 1
    for (uint64_t q = r.q_lo + tid; q < r.q_hi; q += kBlock) {   // q < m
        const uint64_t a = coff[q], b = coff[q + 1];
        if (b > a && a >= r.s && a - r.s < r.cnt) s_pos[a - r.s] = (uint32_t)q + 1u;
    }
    __syncthreads();
    // the position of a slot: the last mark at or below it (marks grow with the
    // slot); in front of the first mark the position before q_lo, whose list
    // began in an earlier tile
    uint32_t mk[kMemPer];
    {
        const uint4* mine = reinterpret_cast<const uint4*>(s_pos + kMemPer * tid);
        const uint4 v0 = mine[0], v1 = mine[1];
        mk[0] = v0.x; mk[1] = v0.y; mk[2] = v0.z; mk[3] = v0.w;
        mk[4] = v1.x; mk[5] = v1.y; mk[6] = v1.z; mk[7] = v1.w;
    }
    uint32_t last = 0;
#pragma unroll
    for (int j = 0; j < kMemPer; ++j) last = std::max(last, mk[j]);
    uint32_t incl = last;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o, kWave);
        if ((int)lane >= o) incl = std::max(incl, y);
    }
    if (lane == kWave - 1) s_w[wave] = incl;
    __syncthreads();
    uint32_t cur = (uint32_t)__shfl_up((int)incl, 1, kWave);
    if (lane == 0) cur = 0u;
    for (uint32_t w = 0; w < wave; ++w) cur = std::max(cur, s_w[w]);
    cur = std::max(cur, (uint32_t)r.q_lo);   // (q_lo - 1) + 1; slot 0 is marked when q_lo == 0
#pragma unroll
    for (int j = 0; j < kMemPer; ++j) {
        cur = std::max(cur, mk[j]);
        pos[j] = cur ? cur - 1u : 0u;
    }
    {
        uint4* mine = reinterpret_cast<uint4*>(s_pos + kMemPer * tid);
        mine[0] = make_uint4(pos[0], pos[1], pos[2], pos[3]);
        mine[1] = make_uint4(pos[4], pos[5], pos[6], pos[7]);
    }
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kBlock) void k_mem_seeds(const uint32_t* __restrict__ len, const uint32_t* __restrict__ lo,
                                                      uint32_t* __restrict__ hi, uint64_t m, uint64_t n, uint64_t L,
                                                      uint64_t max_occ, unsigned long long* __restrict__ words) {
    unsigned long long cand = 0, skip = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t a = lo[i];
        bool skipped;
        const uint32_t c = mem_seed_count(len[i], a, hi[i], n, L, max_occ, skipped);
        if (c == 0u) hi[i] = a;
        cand += c;
        skip += skipped ? 1u : 0u;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        cand += __shfl_down(cand, o, kWave);
        skip += __shfl_down(skip, o, kWave);
    }
    // one pair of atomics per workgroup: every wavefront adding to the same two
    // words (8192 of them for a 1 MiB query) cost 0.1 ms
    __shared__ unsigned long long s_c[kWaves], s_s[kWaves];
    if (lane_id() == 0) {
        s_c[threadIdx.x / kWave] = cand;
        s_s[threadIdx.x / kWave] = skip;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cand = skip = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            cand += s_c[w];
            skip += s_s[w];
        }
        if (cand) atomicAdd(&words[0], cand);
        if (skip) atomicAdd(&words[1], skip);
    }
}

// flagb[t * kBlock + lane of the workgroup]: bit j = candidate t * kMemTile +
// kMemPer * lane + j is left-maximal; tcnt[t] = the tile's survivors
__global__ __launch_bounds__(kBlock) void k_mem_flag(const uint8_t* __restrict__ text, uint64_t n,
                                                     const uint8_t* __restrict__ query, uint64_t m,
                                                     const uint64_t* __restrict__ coff,
                                                     const uint32_t* __restrict__ cand, uint64_t total,
                                                     uint8_t* __restrict__ flagb, int64_t* __restrict__ tcnt) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t pos[kMemPer];
        const MemTile r = mem_tile_positions(coff, m, t, total, s_pos, s_w, s_q, pos);
        // the tile's gathers first, then their use
        uint8_t tb[kMemPer], qb[kMemPer];
        uint64_t p[kMemPer];
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            const uint32_t slot = kMemPer * tid + j;
            p[j] = slot < r.cnt ? mem_clamp_pos(cand[r.s + slot], n) : 0;
        }
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            tb[j] = text[p[j] ? p[j] - 1 : 0];
            qb[j] = query[pos[j] ? pos[j] - 1u : 0u];
        }
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < kMemPer; ++j)
            if (kMemPer * tid + j < r.cnt && mem_left_maximal(pos[j], p[j], qb[j], tb[j])) bits |= 1u << j;
        uint32_t sum;
        (void)mem_block_excl((uint32_t)__popc(bits), s_w, sum);
        flagb[t * kBlock + tid] = (uint8_t)bits;
        if (tid == 0) tcnt[t] = (int64_t)sum;
    }
}

// the bytes Q from i and T from p share, from `start` shared bytes on, by a
// whole wavefront: 512 bytes a step.  Every argument is the same in all lanes.
__device__ __forceinline__ uint64_t mem_extend_wave(const uint8_t* __restrict__ text, uint64_t n,
                                                    const uint8_t* __restrict__ query, uint64_t m, uint64_t i,
                                                    uint64_t p, uint64_t start) {
    const uint64_t tl = p < n ? n - p : 0, ql = i < m ? m - i : 0;
    const uint64_t lim = tl < ql ? tl : ql;
    const uint32_t lane = lane_id();
    for (uint64_t off = start; off < lim; off += (uint64_t)kWave * 8) {
        const uint64_t o = off + (uint64_t)lane * 8;
        bool mis = false;
        uint32_t j = 0;
        if (o < lim) {
            const uint64_t d = load8(text, p + o, n) ^ load8(query, i + o, m);
            if (d) {
                j = (uint32_t)(__builtin_ctzll(d) >> 3);
                mis = o + j < lim;
            }
        }
        const uint64_t bm = __ballot(mis);
        if (bm) {
            const int f = __builtin_ctzll(bm);
            return off + (uint64_t)f * 8 + (uint32_t)__shfl((int)j, f, kWave);
        }
    }
    return lim;
}

// tbase: the inclusive sums of the tile counts.  off is always written; tpos
// and len only when they are given and the total fits out_cap.  lane_words:
// the words a lane compares before it lists its candidate for a wavefront
// (0: every candidate listed, ~0: none).
__global__ __launch_bounds__(kBlock) void k_mem_emit(const uint8_t* __restrict__ text, uint64_t n,
                                                     const uint8_t* __restrict__ query, uint64_t m, uint64_t L,
                                                     const uint64_t* __restrict__ coff,
                                                     const uint32_t* __restrict__ cand, uint64_t total,
                                                     const uint8_t* __restrict__ flagb,
                                                     const int64_t* __restrict__ tbase, uint64_t lane_words,
                                                     uint64_t* __restrict__ off, uint32_t* __restrict__ tpos,
                                                     uint32_t* __restrict__ len, uint64_t out_cap) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint32_t s_rank[kMemTile + 1];   // survivors of the tile in front of each slot; [kMemTile]: all
    __shared__ uint2 s_list[kMemTile];          // (slot, bytes shared so far) of the extensions left to the wavefronts
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    __shared__ uint32_t s_n;
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    const uint64_t mems = (uint64_t)tbase[tiles - 1];
    const bool write = tpos != nullptr && len != nullptr && mems <= out_cap;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t pos[kMemPer];
        const MemTile r = mem_tile_positions(coff, m, t, total, s_pos, s_w, s_q, pos);
        const uint64_t base = t ? (uint64_t)tbase[t - 1] : 0;
        uint32_t bits = flagb[t * kBlock + tid];
        uint32_t sum;
        const uint32_t mine = mem_block_excl((uint32_t)__popc(bits), s_w, sum);
#pragma unroll
        for (int j = 0; j < kMemPer; ++j)
            s_rank[kMemPer * tid + j] = mine + (uint32_t)__popc(bits & ((1u << j) - 1u));
        if (tid == 0) {
            s_rank[kMemTile] = sum;
            s_n = 0u;
        }
        __syncthreads();
        // off of the positions whose list starts here: flags past cnt are 0,
        // so s_rank[cnt] is the tile's sum.  The last tile takes the
        // positions at the very end and off[m].
        const uint64_t q_end = t + 1 == tiles ? m + 1 : r.q_hi;
        for (uint64_t q = r.q_lo + tid; q < q_end; q += kBlock) {
            const uint64_t a = coff[q];
            const uint32_t slot = a >= r.s ? (uint32_t)std::min<uint64_t>(a - r.s, r.cnt) : 0u;
            off[q] = base + s_rank[slot];
        }
        if (write) {
            while (bits) {
                const int j = __builtin_ctz(bits);
                bits &= bits - 1u;
                const uint32_t slot = kMemPer * tid + j;
                const uint64_t i = s_pos[slot];
                const uint64_t p = mem_clamp_pos(cand[r.s + slot], n);
                const uint64_t o = base + s_rank[slot];
                bool done;
                const uint64_t k = mem_extend_steps(
                    i, p, L, n, m, [&](uint64_t x) { return load8(text, x, n); },
                    [&](uint64_t x) { return load8(query, x, m); }, lane_words, done);
                tpos[o] = (uint32_t)p;
                if (done) len[o] = (uint32_t)k;
                else s_list[atomicAdd(&s_n, 1u)] = make_uint2(slot, (uint32_t)k);
            }
            __syncthreads();
            const uint32_t nl = s_n;   // <= the tile's survivors <= kMemTile
            for (uint32_t x = wave; x < nl; x += kWaves) {
                const uint2 it = s_list[x];
                const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.x);
                const uint64_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pos[slot]);
                const uint64_t p =
                    mem_clamp_pos((uint32_t)__builtin_amdgcn_readfirstlane((int)cand[r.s + slot]), n);
                const uint64_t k = mem_extend_wave(text, n, query, m, i, p,
                                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)it.y));
                if (lane == 0) len[base + s_rank[slot]] = (uint32_t)k;
            }
        }
        __syncthreads();   // the next tile writes these arrays
    }
}

// the checks of sa_mems_device, all before any HIP call
static int mem_check_args(const sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                          const uint8_t* d_query, uint64_t m, uint64_t min_len, uint32_t flags, const uint64_t* d_off,
                          const uint32_t* d_tpos, const uint32_t* d_len, const uint64_t* info) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (!d_off) return set_err(SA_E_INVALID, "d_off is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (m > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "m too large");
    if (n && !d_text) return set_err(SA_E_INVALID, "d_text is NULL");
    if (n && !d_sa) return set_err(SA_E_INVALID, "d_sa is NULL");
    if (m && !d_query) return set_err(SA_E_INVALID, "d_query is NULL");
    if (min_len == 0) return set_err(SA_E_INVALID, "min_len is 0");
    if (flags & ~(uint32_t)(SA_MEM_LANE | SA_MEM_WAVE)) return set_err(SA_E_INVALID, "unknown flags %#x", flags);
    if (flags == (SA_MEM_LANE | SA_MEM_WAVE))
        return set_err(SA_E_INVALID, "SA_MEM_LANE and SA_MEM_WAVE exclude each other");
    if (!d_tpos != !d_len) return set_err(SA_E_INVALID, "d_tpos and d_len: both or neither");
    const void* in[3] = {d_text, d_sa, d_query};
    const void* out[3] = {d_off, d_tpos, d_len};
    for (const void* o : out)
        for (const void* i : in)
            if (o && o == i) return set_err(SA_E_INVALID, "an output aliases an input");
    if (d_tpos && ((const void*)d_tpos == (const void*)d_len || (const void*)d_tpos == (const void*)d_off ||
                   (const void*)d_len == (const void*)d_off))
        return set_err(SA_E_INVALID, "two outputs are one buffer");
    return SA_OK;
}

// the host form's outputs, allocated when the total is known
struct MemOwn {
    DevBuf tpos, len;
    bool want = false;   // the caller gave host outputs
};

// Host waits: the seed counts; locate's own (one, more with positions above
// SA_LOCATE_TILE hits); the total.  own: the host form (the emit kernel is
// then launched after the total is known, into buffers made for it).
static int mems_device(sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query,
                       uint64_t m, uint64_t min_len, uint64_t max_occ, uint64_t max_candidates, uint32_t flags,
                       uint64_t* d_off, uint32_t* d_tpos, uint32_t* d_len, uint64_t out_cap, uint64_t* info,
                       hipStream_t s, MemOwn* own = nullptr) {
    SA_TRY(mem_check_args(c, d_text, n, d_sa, d_query, m, min_len, flags, d_off, d_tpos, d_len, info));
    info[0] = info[1] = info[2] = 0;
    SA_HIP(hipSetDevice(c->device));
    auto no_mems = [&]() -> int {
        SA_HIP(hipMemsetAsync(d_off, 0, (m + 1) * 8, s));
        SA_HIP(host_sync(s));
        return SA_OK;
    };
    if (n == 0 || m == 0 || min_len > std::min(n, m)) return no_mems();
    uint64_t* h = reinterpret_cast<uint64_t*>(c->host_words + kMemHostWord);
    const uint32_t sgrid = (uint32_t)std::min<uint64_t>((m + kBlock - 1) / kBlock, (uint64_t)c->cus * 4);
    uint64_t cands = 0;
    LocBuf list;   // coff (m + 1) | tile counts | candidates | flag bytes
    uint64_t* d_coff = nullptr;
    {
        LocBuf seeds;   // candidates, skipped | len | lo | hi
        SA_TRY(seeds.alloc(16 + 3 * m * 4, s));
        unsigned long long* d_words = (unsigned long long*)seeds.p;
        uint32_t* d_slen = (uint32_t*)(d_words + 2);
        uint32_t* d_lo = d_slen + m;
        uint32_t* d_hi = d_lo + m;
        SA_HIP(hipMemsetAsync(d_words, 0, 16, s));
        SA_TRY(match_stats_device(d_text, n, d_sa, d_query, m, min_len, d_slen, d_lo, d_hi, 0, s));
        hipLaunchKernelGGL(k_mem_seeds, dim3(sgrid), dim3(kBlock), 0, s, (const uint32_t*)d_slen, (const uint32_t*)d_lo,
                           d_hi, m, n, min_len, max_occ, d_words);
        SA_HIP(hipGetLastError());
        SA_HIP(hipMemcpyAsync(h, d_words, 16, hipMemcpyDeviceToHost, s));
        SA_HIP(host_sync(s));
        cands = h[0];
        info[1] = cands;
        info[2] = h[1];
        SA_TRACE("mems: m %llu candidates %llu skipped %llu", (unsigned long long)m, (unsigned long long)cands,
                 (unsigned long long)h[1]);
        if (max_candidates && cands > max_candidates) {
            SA_TRY(no_mems());
            return SA_MEM_TOO_MANY;
        }
        if (cands == 0) return no_mems();
        const uint64_t tiles = (cands + kMemTile - 1) / kMemTile;
        SA_TRY(list.alloc((m + 1) * 8 + tiles * 8 + align_up(cands, 4) * 4 + tiles * kBlock, s));
        d_coff = (uint64_t*)list.p;
        uint32_t* d_cand = (uint32_t*)(d_coff + m + 1 + tiles);
        uint64_t got = 0;
        SA_TRY(locate_device(c, n, d_sa, d_lo, d_hi, m, 0, 0, d_coff, d_cand, cands, &got, s));
        if (got != cands)
            return set_err(SA_E_INTERNAL, "mems: locate wrote %llu hits for %llu candidates", (unsigned long long)got,
                           (unsigned long long)cands);
    }
    const uint64_t tiles = (cands + kMemTile - 1) / kMemTile;
    int64_t* d_tcnt = (int64_t*)(d_coff + m + 1);
    const uint32_t* d_cand = (const uint32_t*)(d_tcnt + tiles);
    uint8_t* d_flagb = (uint8_t*)(d_cand + align_up(cands, 4));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)c->cus * kMemGridPerCu);
    hipLaunchKernelGGL(k_mem_flag, dim3(grid), dim3(kBlock), 0, s, d_text, n, d_query, m, (const uint64_t*)d_coff, d_cand,
                       cands, d_flagb, d_tcnt);
    SA_HIP(hipGetLastError());
    SA_TRY(scan_i64<ScanSum>(d_tcnt, tiles, s));
    const uint64_t lane_words = flags & SA_MEM_LANE ? ~0ull : flags & SA_MEM_WAVE ? 0ull : kMemLaneBytes / 8;
    auto emit = [&](uint32_t* tp, uint32_t* ln, uint64_t cap) -> int {
        hipLaunchKernelGGL(k_mem_emit, dim3(grid), dim3(kBlock), 0, s, d_text, n, d_query, m, min_len,
                           (const uint64_t*)d_coff, d_cand, cands, (const uint8_t*)d_flagb, (const int64_t*)d_tcnt,
                           lane_words, d_off, tp, ln, cap);
        SA_HIP(hipGetLastError());
        return SA_OK;
    };
    if (!own) SA_TRY(emit(d_tpos, d_len, out_cap));
    SA_HIP(hipMemcpyAsync(h + 2, d_tcnt + (tiles - 1), 8, hipMemcpyDeviceToHost, s));
    SA_HIP(host_sync(s));
    info[0] = h[2];
    if (own) {
        const bool fits = own->want && info[0] > 0 && info[0] <= out_cap;
        if (fits) {
            SA_TRY(own->tpos.alloc(align_up(info[0], 64) * 4));
            SA_TRY(own->len.alloc(align_up(info[0], 64) * 4));
        }
        SA_TRY(emit(fits ? own->tpos.as<uint32_t>() : nullptr, fits ? own->len.as<uint32_t>() : nullptr, out_cap));
        SA_HIP(host_sync(s));
    }
    return SA_OK;
}

// host in, host out (sa_mems), over the steps of sa_host.h.  The device form
// sizes first; the outputs are allocated when the total is known.
static int mems_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* query, uint64_t m,
                     uint64_t min_len, uint64_t max_occ, uint64_t max_candidates, uint32_t flags, uint64_t* off_out,
                     void* tpos_out, void* len_out, uint64_t out_cap, uint64_t* info) {
    SA_TRY(check_width(sa_width));
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (!off_out) return set_err(SA_E_INVALID, "off_out is NULL");
    SA_TRY(check_n32(n));
    if (m > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "m too large");
    if (n && !text) return set_err(SA_E_INVALID, "text is NULL");
    if (n && !sa) return set_err(SA_E_INVALID, "sa is NULL");
    if (m && !query) return set_err(SA_E_INVALID, "query is NULL");
    if (min_len == 0) return set_err(SA_E_INVALID, "min_len is 0");
    if (flags & ~(uint32_t)(SA_MEM_LANE | SA_MEM_WAVE)) return set_err(SA_E_INVALID, "unknown flags %#x", flags);
    if (flags == (SA_MEM_LANE | SA_MEM_WAVE))
        return set_err(SA_E_INVALID, "SA_MEM_LANE and SA_MEM_WAVE exclude each other");
    if (!tpos_out != !len_out) return set_err(SA_E_INVALID, "tpos_out and len_out: both or neither");
    const void* in[3] = {text, sa, query};
    const void* out[3] = {off_out, tpos_out, len_out};
    for (const void* o : out)
        for (const void* i : in)
            if (o && o == i) return set_err(SA_E_INVALID, "an output aliases an input");
    info[0] = info[1] = info[2] = 0;
    if (n == 0 || m == 0 || min_len > std::min(n, m)) {
        std::memset(off_out, 0, (m + 1) * 8);
        return SA_OK;
    }
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_text, d_sa, d_query, d_off;
    MemOwn own;
    own.want = tpos_out != nullptr;
    SA_TRY(d_text.alloc(align_up(n + 1, 256)));
    SA_TRY(d_sa.alloc(align_up(n + 1, 64) * 4));
    SA_TRY(d_query.alloc(align_up(m + 1, 256)));
    SA_TRY(d_off.alloc(align_up(m + 1, 64) * 8));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}, {d_query.p, query, m}}));
    const int rc = mems_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_query.as<uint8_t>(), m, min_len,
                               max_occ, max_candidates, flags, d_off.as<uint64_t>(), nullptr, nullptr, out_cap, info,
                               nullptr, &own);
    if (rc < 0) return rc;
    SA_HIP(hipMemcpyAsync(off_out, d_off.p, (m + 1) * 8, hipMemcpyDeviceToHost, nullptr));
    SA_HIP(host_sync(nullptr));
    if (rc == SA_OK && own.tpos.p) {
        SA_TRY(copy_d2h(tpos_out, own.tpos.as<uint32_t>(), info[0], sa_width, nullptr));
        SA_TRY(copy_d2h(len_out, own.len.as<uint32_t>(), info[0], sa_width, nullptr));
    }
    return rc;
}

}  // namespace sa

extern "C" {

int sa_mems_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query,
                   uint64_t m, uint64_t min_len, uint64_t max_occ, uint64_t max_candidates, uint32_t flags,
                   uint64_t* d_off, uint32_t* d_tpos, uint32_t* d_len, uint64_t out_cap, uint64_t info[SA_MEM_INFO],
                   void* stream) {
    return sa::mems_device(ctx, d_text, n, d_sa, d_query, m, min_len, max_occ, max_candidates, flags, d_off, d_tpos,
                           d_len, out_cap, info, (hipStream_t)stream);
}

int sa_mems(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* query, uint64_t m,
            uint64_t min_len, uint64_t max_occ, uint64_t max_candidates, uint32_t flags, uint64_t* off_out,
            void* tpos_out, void* len_out, uint64_t out_cap, uint64_t info[SA_MEM_INFO]) {
    return sa::mems_host(text, n, sa, sa_width, query, m, min_len, max_occ, max_candidates, flags, off_out, tpos_out,
                         len_out, out_cap, info);
}

}  // extern "C"

#endif   // __HIPCC__
