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
// The HIP part needs sa_match.h, sa_locate.h and sa_query.h (the candidate
// tiles, CandList) before it.
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

__global__ __launch_bounds__(kBlock) void k_mem_seeds(const uint32_t* __restrict__ len, const uint32_t* __restrict__ lo,
                                                      uint32_t* __restrict__ hi, uint64_t m, uint64_t n, uint64_t L,
                                                      uint64_t max_occ, unsigned long long* __restrict__ words) {
    unsigned long long v[2] = {0, 0};   // candidates, skipped
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t a = lo[i];
        bool skipped;
        const uint32_t c = mem_seed_count(len[i], a, hi[i], n, L, max_occ, skipped);
        if (c == 0u) hi[i] = a;
        v[0] += c;
        v[1] += skipped ? 1u : 0u;
    }
    block_sum_u64(v, words);
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

static int mem_check_values(uint64_t min_len, uint32_t flags) {
    if (min_len == 0) return set_err(SA_E_INVALID, "min_len is 0");
    SA_TRY(check_flags(flags, SA_MEM_LANE | SA_MEM_WAVE));
    return check_exclusive(flags, SA_MEM_LANE, SA_MEM_WAVE, "SA_MEM_LANE", "SA_MEM_WAVE");
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
    SA_TRY(mem_check_values(min_len, flags));
    if (!d_tpos != !d_len) return set_err(SA_E_INVALID, "d_tpos and d_len: both or neither");
    SA_TRY(check_no_alias({d_off, d_tpos, d_len}, {d_text, d_sa, d_query}));
    return check_distinct({d_off, d_tpos, d_len});
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
    if (n == 0 || m == 0 || min_len > std::min(n, m)) return empty_csr(d_off, m, s);
    uint64_t* h = host_u64<kHwMem, 3>(c);
    const uint32_t sgrid = (uint32_t)std::min<uint64_t>((m + kBlock - 1) / kBlock, (uint64_t)c->cus * 4);
    CandList list;
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
        info[1] = h[0];
        info[2] = h[1];
        SA_TRACE("mems: m %llu candidates %llu skipped %llu", (unsigned long long)m, (unsigned long long)h[0],
                 (unsigned long long)h[1]);
        const int rc = list.fill(c, "mems", n, d_sa, d_lo, d_hi, m, h[0], max_candidates, SA_MEM_TOO_MANY, d_off, m,
                                 0, 0, s);
        if (rc || !list.tiles) return rc;
    }
    hipLaunchKernelGGL(k_mem_flag, dim3(list.grid), dim3(kBlock), 0, s, d_text, n, d_query, m, (const uint64_t*)list.coff,
                       (const uint32_t*)list.cand, list.cands, list.flagb, list.tcnt);
    SA_HIP(hipGetLastError());
    SA_TRY(list.scan(s));
    const uint64_t lane_words = flags & SA_MEM_LANE ? ~0ull : flags & SA_MEM_WAVE ? 0ull : kMemLaneBytes / 8;
    auto emit = [&](uint32_t* tp, uint32_t* ln, uint64_t cap) -> int {
        hipLaunchKernelGGL(k_mem_emit, dim3(list.grid), dim3(kBlock), 0, s, d_text, n, d_query, m, min_len,
                           (const uint64_t*)list.coff, (const uint32_t*)list.cand, list.cands,
                           (const uint8_t*)list.flagb, (const int64_t*)list.tcnt, lane_words, d_off, tp, ln, cap);
        SA_HIP(hipGetLastError());
        return SA_OK;
    };
    if (!own) SA_TRY(emit(d_tpos, d_len, out_cap));
    SA_TRY(list.total(h + 2, s, &info[0]));
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
    SA_TRY(mem_check_values(min_len, flags));
    if (!tpos_out != !len_out) return set_err(SA_E_INVALID, "tpos_out and len_out: both or neither");
    SA_TRY(check_no_alias({off_out, tpos_out, len_out}, {text, sa, query}));
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
