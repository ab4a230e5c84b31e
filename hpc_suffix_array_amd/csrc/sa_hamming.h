// sa_hamming.h -- k-mismatch pattern search over a built suffix array
// (sa_hamming / sa_hamming_device of include/sa_hip.h).
//
// Definition.  Pattern P of m bytes, a budget k with 0 <= k <= SA_HAMMING_MAX_K
// = 255, text T of n bytes.  An occurrence is a text position p with
// p + m <= n and d(p) <= k, where d(p) = #{ t : P[t] != T[p + t] }.  Bytes are
// sa_find's: binary-safe, 0x00 and 0xFF are ordinary, lengths are explicit.
// The empty pattern occurs at every p in [0, n) with distance 0 (sa_find's
// [0, n)); m > n or n == 0 gives no occurrence; m <= k is answered as defined
// (every p <= n - m is an occurrence).  One k per call.
// Output: CSR over the queries as sa_locate_device writes it: off (nq + 1
// uint64, off[0] = 0, the total is off[nq]), pos (uint32, ascending inside each
// query, every occurrence exactly once) and dist (uint8, d(p) of the same slot;
// may be NULL).
//
// Pigeonhole seeds.  Piece j (j = 0 .. k) of a pattern is P[b_j, b_{j+1}) with
// b_j = floor(j m / (k + 1)) (the product in 64 bits).  If d(p) <= k one of the
// k + 1 pieces has no mismatch at p, so p + b_j is among that piece's exact
// occurrences.  Pieces are contiguous and the patterns are contiguous in d_pat,
// so the piece boundaries of the batch are one non-decreasing array of
// nq (k + 1) + 1 offsets into d_pat: what sa_find_device takes.  An empty piece
// (m < k + 1) gets sa_find's [0, n).
//
// The verify also removes the duplicates.  A candidate is (query q, piece j,
// hit h) with start p = h - b_j; it is invalid when h >= n, h < b_j or
// p + m > n.  It is kept exactly when it is valid, d(p) <= k, and j is the
// first piece of the pattern that matches T exactly at p.  Every occurrence is
// then listed once without a sort, a hash or an atomic: the first exactly
// matching piece of an occurrence is a piece whose hit list holds it (locate is
// not capped here), and no other candidate of the same (q, p) passes.  When a
// piece is empty piece 0 is (b_1 = floor(m / (k + 1)) = 0), it matches
// everywhere, and its hits are all of [0, n): no special path for m <= k.
// The loop runs the pieces in order; it stops as a duplicate at the first piece
// j' < j without a mismatch and as too far as soon as the running count passes
// k, so it reads no more than it must.
//
//   k_ham_pieces   the piece offsets.
//   find_device    on the pieces (sa_find.h): [lo, hi) per piece.
//   k_ham_count    the candidates, the sum of hi - lo; the host reads it (the
//                  first wait), applies max_candidates and sizes the list.
//   locate_device  with SA_LOCATE_SA_ORDER: cand[coff[g] .. coff[g + 1]) are
//                  the hits of piece g = q (k + 1) + j.
//   k_ham_verify   the hot kernel.  A persistent grid over tiles of kMemTile
//                  candidates, their pieces from coff by mem_tile_positions
//                  (sa_query.h), the rule above by 8-byte words (load8), one
//                  flag byte per lane and a count per tile.  A lane verifies
//                  the candidates of patterns of up to kHamLaneBytes bytes;
//                  those of longer patterns go to an LDS list and the
//                  wavefronts take them one each, 512 bytes a step, the
//                  mismatches of a step counted by four ballots over the bits
//                  of the lanes' counts (sa_query.h's mem_wave_turns).
//                  SA_HAMMING_LANE / SA_HAMMING_WAVE force one path.
//   scan           scan_i64<ScanSum> over the tile counts; the host reads the
//                  total (a wait).
//   k_ham_emit     stable compaction of the surviving starts p, and each
//                  query's [lo2, hi2) in the survivor array from the ranks at
//                  the piece boundaries q (k + 1).
//   locate_device_n over the survivor array and those intervals: off and the
//                  sorted pos, and the sizing call's behaviour.  Its limits
//                  are inherited: at most 2^32 - 1 occurrences in all.
//   k_ham_dist     when dist is wanted: d(p) of the survivors in output order,
//                  the owners from off by mem_tile_positions, the same two
//                  paths.  Recomputing keeps the 32-bit sort as it is.
//
// The piece bounds, the word count, the validity test and the verify rule
// compile on the host: tests/cpp/hamming_check.cpp checks them against the
// sliding-window definition.  Measurements and the resource report: DESIGN.md
// section 21.  The HIP part needs sa_find.h, sa_locate.h and sa_query.h
// (the candidate tiles, CandList, sort_lists) before it.
#pragma once
#include <stdint.h>

#include "sa_search.h"   // SA_HD

namespace sa {

// the largest budget (= SA_HAMMING_MAX_K); distances fit a byte
constexpr uint32_t kHamMaxK = 255;
// patterns of up to kHamLaneBytes bytes are verified by a lane, longer ones
// by a wavefront (auto mode).  Measured, DESIGN.md section 21: a tile's
// hand-over list is worked off by its four wavefronts, and every candidate of a
// long pattern is on it, so the lanes stay ahead up to 8192 bytes.
constexpr uint64_t kHamLaneBytes = 8192;

// what the verify says of a candidate
enum HamVerdict : int {
    kHamKeep = 0,        // an occurrence, and this candidate is the one that lists it
    kHamInvalid = 1,     // h >= n, h < b_j or p + m > n
    kHamDuplicate = 2,   // an earlier piece matches exactly at p: its candidate lists p
    kHamTooFar = 3,      // d(p) > k
    kHamNoSeed = 4       // piece j does not match at p (not a hit of piece j: an invalid SA)
};

// b_j = floor(j m / (k + 1)), j in [0, k + 1]; j m < 2^64 for j <= 256, m < 2^56
SA_HD uint64_t ham_piece_bound(uint64_t m, uint32_t k, uint32_t j) { return (uint64_t)j * m / ((uint64_t)k + 1u); }

// the mismatching bytes among those of mask (each byte 0x00 or 0xFF) of two
// words whose xor is x: bit 7 of a byte of ((x & 0x7F..) + 0x7F..) | x is set
// iff the byte of x is not zero
SA_HD uint32_t ham_word_mismatches(uint64_t x, uint64_t mask) {
    const uint64_t lo7 = 0x7F7F7F7F7F7F7F7Full;
    x &= mask;
    return (uint32_t)__builtin_popcountll((((x & lo7) + lo7) | x) & ~lo7);
}

// the first `bytes` bytes of a word (bytes >= 8: all of it)
SA_HD uint64_t ham_low_mask(uint64_t bytes) { return bytes >= 8 ? ~0ull : (1ull << (8 * bytes)) - 1ull; }

// start p = h - bj of the candidate (hit h of the piece that begins at byte bj
// of a pattern of m bytes); false when it is invalid.  A hit >= n (an invalid
// SA) reads as invalid.
SA_HD bool ham_candidate_start(uint64_t h, uint64_t bj, uint64_t m, uint64_t n, uint64_t& p) {
    if (h >= n || h < bj) return false;
    p = h - bj;
    return m <= n && p <= n - m;
}

// mismatches of P[b, e) against T[p + b, p + e) by 8-byte words, the last word
// masked; the count stops growing once it is above `budget`.  text_word(x) /
// pat_word(x): the little-endian 8 bytes at text position x / at byte x of the
// pattern, zero at or past the end (load8).  Needs p + e <= n and e <= m: no
// word starts at or past p + e or e.
template <class TextWord, class PatWord>
SA_HD uint32_t ham_count_lane(uint64_t p, uint64_t b, uint64_t e, uint32_t budget, const TextWord& text_word,
                              const PatWord& pat_word) {
    uint32_t c = 0;
    for (uint64_t off = b; off < e && c <= budget; off += 8)
        c += ham_word_mismatches(text_word(p + off) ^ pat_word(off), ham_low_mask(e - off));
    return c;
}

// The rule over the pieces in order.  piece_count(b, e, budget): the
// mismatches of P[b, e) at p, exact up to `budget` (above it any value above
// it).  The bounds advance by q = m / (k + 1) plus the carry of the remainders
// (no division per piece): b_{j+1} - b_j = q + [(j r) mod (k + 1) + r >= k + 1]
// with r = m mod (k + 1).  dist is written for kHamKeep alone.
template <class PieceCount>
SA_HD HamVerdict ham_verify_pieces(uint64_t m, uint32_t k, uint32_t j, const PieceCount& piece_count, uint32_t& dist) {
    const uint64_t k1 = (uint64_t)k + 1u, q = m / k1, r = m - q * k1;
    uint64_t b = 0, acc = 0;
    uint32_t d = 0;
    for (uint32_t jj = 0; jj <= k; ++jj) {
        acc += r;
        uint64_t e = b + q;
        if (acc >= k1) {
            acc -= k1;
            ++e;
        }
        const uint32_t c = piece_count(b, e, k - d);
        if (jj < j && c == 0) return kHamDuplicate;
        if (jj == j && c != 0) return kHamNoSeed;
        d += c;
        if (d > k) return kHamTooFar;
        b = e;
    }
    dist = d;
    return kHamKeep;
}

// a candidate (piece j, hit h) of a pattern of m bytes, by a lane
template <class TextWord, class PatWord>
SA_HD HamVerdict ham_verify(uint64_t n, uint64_t m, uint32_t k, uint32_t j, uint64_t h, const TextWord& text_word,
                            const PatWord& pat_word, uint64_t& p, uint32_t& dist) {
    if (!ham_candidate_start(h, ham_piece_bound(m, k, j), m, n, p)) return kHamInvalid;
    const uint64_t p0 = p;
    return ham_verify_pieces(
        m, k, j, [&](uint64_t b, uint64_t e, uint32_t budget) { return ham_count_lane(p0, b, e, budget, text_word, pat_word); },
        dist);
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

namespace sa {

static_assert(SA_HAMMING_MAX_K == 255 && SA_HAMMING_TOO_MANY == 1 && SA_HAMMING_LANE == 1u && SA_HAMMING_WAVE == 2u &&
                  SA_HAMMING_INFO == 3,
              "sa_hip.h states these");
static_assert(kHamMaxK == SA_HAMMING_MAX_K, "the header's largest budget");
static_assert(kHamLaneBytes % 8 == 0, "whole words");

__global__ __launch_bounds__(kBlock) void k_ham_pieces(const uint64_t* __restrict__ off, uint64_t nq, uint64_t pat_bytes,
                                                       uint32_t k, uint64_t* __restrict__ poff) {
    const uint64_t k1 = (uint64_t)k + 1u, np = nq * k1;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g <= np; g += (uint64_t)gridDim.x * kBlock) {
        const uint64_t q = g < np ? g / k1 : nq - 1;
        uint64_t a, m;
        find_pattern(off, q, pat_bytes, a, m);
        poff[g] = g < np ? a + ham_piece_bound(m, k, (uint32_t)(g - q * k1)) : a + m;   // <= pat_bytes
    }
}

// word[0] += the hits of the pieces, counted as locate_device counts them
__global__ __launch_bounds__(kBlock) void k_ham_count(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                      uint64_t np, uint64_t n, unsigned long long* __restrict__ word) {
    unsigned long long c[1] = {0};
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < np; g += (uint64_t)gridDim.x * kBlock)
        c[0] += locate_count(lo[g], hi[g], n, 0);
    block_sum_u64(c, word);
}

// The patterns and the text as the verify reads them.
struct HamIn {
    const uint8_t* __restrict__ text;
    uint64_t n;
    const uint8_t* __restrict__ pat;
    uint64_t pat_bytes;
    const uint64_t* __restrict__ pat_off;
};

// mismatches of P[b, e) (P = bytes [pa, pa + m) of pat) at text position p by
// a whole wavefront, 512 bytes a step; every argument is the same in all
// lanes, and so is the result.  A lane's count of a step is at most 8: four
// ballots over its bits.
__device__ __forceinline__ uint32_t ham_count_wave(const HamIn& in, uint64_t pa, uint64_t p, uint64_t b, uint64_t e,
                                                   uint32_t budget) {
    const uint32_t lane = lane_id();
    uint32_t c = 0;
    for (uint64_t off = b; off < e && c <= budget; off += (uint64_t)kWave * 8) {
        const uint64_t o = off + (uint64_t)lane * 8;
        uint32_t x = 0;
        if (o < e)
            x = ham_word_mismatches(load8(in.text, p + o, in.n) ^ load8(in.pat, pa + o, in.pat_bytes),
                                    ham_low_mask(e - o));
#pragma unroll
        for (int bit = 0; bit < 4; ++bit)
            c += (uint32_t)__builtin_popcountll(__ballot((x >> bit) & 1u)) << bit;
    }
    return c;
}

// candidate (piece j, hit h) of the pattern at bytes [pa, pa + m) of pat, by a
// lane (WAVE = false) or by a wavefront with uniform arguments
template <bool WAVE>
__device__ __forceinline__ HamVerdict ham_verify_dev(const HamIn& in, uint32_t k, uint64_t pa, uint64_t m, uint32_t j,
                                                     uint64_t h) {
    uint32_t dist;
    uint64_t p;
    if constexpr (WAVE) {
        if (!ham_candidate_start(h, ham_piece_bound(m, k, j), m, in.n, p)) return kHamInvalid;
        const uint64_t p0 = p;
        return ham_verify_pieces(
            m, k, j, [&](uint64_t b, uint64_t e, uint32_t budget) { return ham_count_wave(in, pa, p0, b, e, budget); },
            dist);
    } else {
        return ham_verify(in.n, m, k, j, h, [&](uint64_t x) { return load8(in.text, x, in.n); },
                          [&](uint64_t x) { return load8(in.pat, pa + x, in.pat_bytes); }, p, dist);
    }
}

// flagb[t * kBlock + lane of the workgroup]: bit j = candidate t * kMemTile +
// kMemPer * lane + j is kept; tcnt[t] = the tile's survivors.  coff: the np + 1
// offsets of the pieces' hit lists; lane_bytes: the longest pattern a lane
// verifies (0: only the empty ones, ~0: all).
__global__ __launch_bounds__(kBlock) void k_ham_verify(HamIn in, uint32_t k, const uint64_t* __restrict__ coff,
                                                       uint64_t np, const uint32_t* __restrict__ cand, uint64_t total,
                                                       uint64_t lane_bytes, uint8_t* __restrict__ flagb,
                                                       int64_t* __restrict__ tcnt) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint16_t s_list[kMemTile];   // the slots left to the wavefronts
    __shared__ uint32_t s_keep[kBlock];     // their verdicts, a byte of flags per lane
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    __shared__ uint32_t s_n;
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t k1 = k + 1u;
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        if (tid == 0) s_n = 0u;
        s_keep[tid] = 0u;
        uint32_t pos[kMemPer];
        const MemTile r = mem_tile_positions(coff, np, t, total, s_pos, s_w, s_q, pos);
        // the tile's gathers first, then their use
        uint32_t h[kMemPer];
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            const uint32_t slot = kMemPer * tid + j;
            h[j] = slot < r.cnt ? cand[r.s + slot] : 0u;
        }
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            const uint32_t slot = kMemPer * tid + j;
            if (slot >= r.cnt) continue;
            const uint32_t q = pos[j] / k1;
            uint64_t pa, m;
            find_pattern(in.pat_off, q, in.pat_bytes, pa, m);
            if (m > lane_bytes) s_list[atomicAdd(&s_n, 1u)] = (uint16_t)slot;   // < kMemTile entries
            else if (ham_verify_dev<false>(in, k, pa, m, pos[j] - q * k1, h[j]) == kHamKeep) bits |= 1u << j;
        }
        __syncthreads();
        // s_n <= cnt <= kMemTile
        mem_wave_turns(
            s_n, [&](uint32_t x) { return s_list[x]; }, s_pos, cand + r.s,
            [&](uint32_t, uint32_t slot, uint32_t g, uint32_t hh) {
                const uint32_t q = g / k1;
                uint64_t pa, m;
                find_pattern(in.pat_off, q, in.pat_bytes, pa, m);
                const HamVerdict v = ham_verify_dev<true>(in, k, pa, m, g - q * k1, hh);
                if (lane == 0 && v == kHamKeep) atomicOr(&s_keep[slot / kMemPer], 1u << (slot % kMemPer));
            });
        __syncthreads();
        bits |= s_keep[tid];
        uint32_t sum;
        (void)mem_block_excl((uint32_t)__popc(bits), s_w, sum);
        flagb[t * kBlock + tid] = (uint8_t)bits;
        if (tid == 0) tcnt[t] = (int64_t)sum;
    }
}

// tbase: the inclusive sums of the tile counts.  surv (may be NULL: the sizing
// call) takes the starts of the kept candidates in candidate order; lo2 / hi2
// take each query's range in surv, from the ranks at the piece boundaries
// q (k + 1).
__global__ __launch_bounds__(kBlock) void k_ham_emit(HamIn in, uint32_t k, const uint64_t* __restrict__ coff, uint64_t np,
                                                     const uint32_t* __restrict__ cand, uint64_t total,
                                                     const uint8_t* __restrict__ flagb,
                                                     const int64_t* __restrict__ tbase, uint32_t* __restrict__ surv,
                                                     uint32_t* __restrict__ lo2, uint32_t* __restrict__ hi2) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint32_t s_rank[kMemTile + 1];   // survivors of the tile in front of each slot; [kMemTile]: all
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t k1 = k + 1u;
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t pos[kMemPer];
        const MemTile r = mem_tile_positions(coff, np, t, total, s_pos, s_w, s_q, pos);
        const uint64_t base = t ? (uint64_t)tbase[t - 1] : 0;
        uint32_t bits = flagb[t * kBlock + tid];
        uint32_t sum;
        const uint32_t mine = mem_block_excl((uint32_t)__popc(bits), s_w, sum);
#pragma unroll
        for (int j = 0; j < kMemPer; ++j)
            s_rank[kMemPer * tid + j] = mine + (uint32_t)__popc(bits & ((1u << j) - 1u));
        if (tid == 0) s_rank[kMemTile] = sum;
        __syncthreads();
        // the pieces whose list starts here (flags past cnt are 0, so
        // s_rank[cnt] is the tile's sum); the last tile takes those at the
        // very end and the end of the last query
        const uint64_t g_end = t + 1 == tiles ? np + 1 : r.q_hi;
        for (uint64_t g = r.q_lo + tid; g < g_end; g += kBlock) {
            const uint64_t q = g / k1;
            if (g != q * k1) continue;
            const uint64_t a = coff[g];
            const uint32_t slot = a >= r.s ? (uint32_t)std::min<uint64_t>(a - r.s, r.cnt) : 0u;
            const uint32_t at = (uint32_t)(base + s_rank[slot]);   // the host stops above 2^32 - 1 survivors
            if (g < np) lo2[q] = at;
            if (q > 0) hi2[q - 1] = at;
        }
        if (surv) {
            while (bits) {
                const int j = __builtin_ctz(bits);
                bits &= bits - 1u;
                const uint32_t slot = kMemPer * tid + j;
                const uint32_t g = s_pos[slot], q = g / k1;
                uint64_t pa, m;
                find_pattern(in.pat_off, q, in.pat_bytes, pa, m);
                // kept: h >= b_j
                surv[base + s_rank[slot]] = cand[r.s + slot] - (uint32_t)ham_piece_bound(m, k, g - q * k1);
            }
        }
        __syncthreads();   // the next tile writes these arrays
    }
}

// dist[x] = d(pos[x]) for the `total` occurrences in output order; off: the
// nq + 1 offsets of the output.  Two paths as the verify's.
__global__ __launch_bounds__(kBlock) void k_ham_dist(HamIn in, const uint64_t* __restrict__ off, uint64_t nq,
                                                     const uint32_t* __restrict__ pos_out, uint64_t total,
                                                     uint64_t lane_bytes, uint8_t* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint16_t s_list[kMemTile];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    __shared__ uint32_t s_n;
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        if (tid == 0) s_n = 0u;
        uint32_t own[kMemPer];
        const MemTile r = mem_tile_positions(off, nq, t, total, s_pos, s_w, s_q, own);
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            const uint32_t slot = kMemPer * tid + j;
            if (slot >= r.cnt) continue;
            uint64_t pa, m;
            find_pattern(in.pat_off, own[j], in.pat_bytes, pa, m);
            if (m > lane_bytes) {
                s_list[atomicAdd(&s_n, 1u)] = (uint16_t)slot;
                continue;
            }
            const uint64_t p = pos_out[r.s + slot];
            uint32_t d = 0;
            if (p < in.n && m <= in.n - p)   // an occurrence; anything else reads nothing
                d = ham_count_lane(p, 0, m, kHamMaxK, [&](uint64_t x) { return load8(in.text, x, in.n); },
                                   [&](uint64_t x) { return load8(in.pat, pa + x, in.pat_bytes); });
            dist[r.s + slot] = (uint8_t)std::min<uint32_t>(d, kHamMaxK);
        }
        __syncthreads();
        mem_wave_turns(
            s_n, [&](uint32_t x) { return s_list[x]; }, s_pos, pos_out + r.s,
            [&](uint32_t, uint32_t slot, uint32_t q, uint32_t p) {
                uint64_t pa, m;
                find_pattern(in.pat_off, q, in.pat_bytes, pa, m);
                uint32_t d = 0;
                if (p < in.n && m <= in.n - p) d = ham_count_wave(in, pa, p, 0, m, kHamMaxK);
                if (lane == 0) dist[r.s + slot] = (uint8_t)std::min<uint32_t>(d, kHamMaxK);
            });
        __syncthreads();   // the next tile writes these arrays
    }
}

static int ham_check_sizes(uint64_t nq, uint64_t k) {
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (k > SA_HAMMING_MAX_K) return set_err(SA_E_INVALID, "k is above SA_HAMMING_MAX_K = %d", SA_HAMMING_MAX_K);
    if (nq * (k + 1) > 0xFFFFFFFFull)
        return set_err(SA_E_INVALID, "nq (k + 1) = %llu pieces are more than 2^32 - 1", (unsigned long long)(nq * (k + 1)));
    return SA_OK;
}
static int ham_check_flags(uint32_t flags) {
    SA_TRY(check_flags(flags, SA_HAMMING_LANE | SA_HAMMING_WAVE));
    return check_exclusive(flags, SA_HAMMING_LANE, SA_HAMMING_WAVE, "SA_HAMMING_LANE", "SA_HAMMING_WAVE");
}

// the checks of sa_hamming_device, all before any HIP call
static int ham_check_args(const sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                          const uint8_t* d_pat, uint64_t pat_bytes, const uint64_t* d_pat_off, uint64_t nq, uint64_t k,
                          uint32_t flags, const uint64_t* d_off, const uint32_t* d_pos, const uint8_t* d_dist,
                          const uint64_t* info) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (!d_off) return set_err(SA_E_INVALID, "d_off is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    SA_TRY(ham_check_sizes(nq, k));
    if (n && !d_text) return set_err(SA_E_INVALID, "d_text is NULL");
    if (n && !d_sa) return set_err(SA_E_INVALID, "d_sa is NULL");
    if (pat_bytes && !d_pat) return set_err(SA_E_INVALID, "d_pat is NULL");
    if (nq && !d_pat_off) return set_err(SA_E_INVALID, "d_pat_off is NULL");
    SA_TRY(ham_check_flags(flags));
    if (d_dist && !d_pos) return set_err(SA_E_INVALID, "d_dist without d_pos");
    SA_TRY(check_no_alias({d_off, d_pos, d_dist}, {d_text, d_sa, d_pat, d_pat_off}));
    return check_distinct({d_off, d_pos, d_dist});
}

// the host form's outputs, allocated when the total is known
struct HamOwn {
    DevBuf pos, dist;
    bool want_pos = false, want_dist = false;   // the caller gave host outputs
};

// Host waits: the candidate count; locate_device's own over the pieces (one,
// two when a piece has more than SA_LOCATE_TILE hits); the total;
// locate_device_n's own over the survivors (one, more when a query has more
// than SA_LOCATE_TILE occurrences); one at the end when distances are written.
static int hamming_device(sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                          uint64_t pat_bytes, const uint64_t* d_pat_off, uint64_t nq, uint64_t k, uint64_t max_candidates,
                          uint32_t flags, uint64_t* d_off, uint32_t* d_pos, uint8_t* d_dist, uint64_t out_cap,
                          uint64_t* info, hipStream_t s, HamOwn* own = nullptr) {
    SA_TRY(ham_check_args(c, d_text, n, d_sa, d_pat, pat_bytes, d_pat_off, nq, k, flags, d_off, d_pos, d_dist, info));
    const uint64_t np = nq * (k + 1);
    info[0] = info[1] = 0;
    info[2] = np;
    SA_HIP(hipSetDevice(c->device));
    if (nq == 0 || n == 0) return empty_csr(d_off, nq, s);
    uint64_t* h = host_u64<kHwHamming, 2>(c);
    // no byte of an empty buffer is read (load8 ends at pat_bytes): any pointer serves
    const HamIn in{d_text, n, d_pat ? d_pat : d_text, pat_bytes, d_pat_off};
    const uint32_t kk = (uint32_t)k;
    const uint32_t pgrid = (uint32_t)std::min<uint64_t>((np + kBlock) / kBlock, (uint64_t)c->cus * 8);
    CandList list;   // extra: lo2 | hi2
    {
        LocBuf seeds;   // the candidate count (16 bytes) | piece offsets (np + 1) | lo | hi
        SA_TRY(seeds.alloc(16 + (np + 1) * 8 + 2 * np * 4, s));
        unsigned long long* d_word = (unsigned long long*)seeds.p;
        uint64_t* d_poff = (uint64_t*)(d_word + 2);
        uint32_t* d_lo = (uint32_t*)(d_poff + np + 1);
        uint32_t* d_hi = d_lo + np;
        SA_HIP(hipMemsetAsync(d_word, 0, 16, s));
        hipLaunchKernelGGL(k_ham_pieces, dim3(pgrid), dim3(kBlock), 0, s, d_pat_off, nq, pat_bytes, kk, d_poff);
        SA_HIP(hipGetLastError());
        SA_TRY(find_device(d_text, n, d_sa, in.pat, pat_bytes, d_poff, np, d_lo, d_hi, 0, s));
        hipLaunchKernelGGL(k_ham_count, dim3(pgrid), dim3(kBlock), 0, s, (const uint32_t*)d_lo, (const uint32_t*)d_hi, np,
                           n, d_word);
        SA_HIP(hipGetLastError());
        SA_HIP(hipMemcpyAsync(h, d_word, 8, hipMemcpyDeviceToHost, s));
        SA_HIP(host_sync(s));
        info[1] = h[0];
        SA_TRACE("hamming: nq %llu k %u pieces %llu candidates %llu", (unsigned long long)nq, kk, (unsigned long long)np,
                 (unsigned long long)h[0]);
        const int rc = list.fill(c, "hamming", n, d_sa, d_lo, d_hi, np, h[0], max_candidates, SA_HAMMING_TOO_MANY,
                                 d_off, nq, SA_LOCATE_SA_ORDER, 2 * nq * 4, s);
        if (rc || !list.tiles) return rc;
    }
    uint32_t *d_lo2 = (uint32_t*)list.extra, *d_hi2 = d_lo2 + nq;
    const uint64_t lane_bytes = flags & SA_HAMMING_LANE ? ~0ull : flags & SA_HAMMING_WAVE ? 0ull : kHamLaneBytes;
    hipLaunchKernelGGL(k_ham_verify, dim3(list.grid), dim3(kBlock), 0, s, in, kk, (const uint64_t*)list.coff, np,
                       (const uint32_t*)list.cand, list.cands, lane_bytes, list.flagb, list.tcnt);
    SA_HIP(hipGetLastError());
    SA_TRY(list.scan(s));
    SA_TRY(list.total(h + 1, s, &info[0]));
    const uint64_t total = info[0];
    if (total == 0) return empty_csr(d_off, nq, s);
    if (total > 0xFFFFFFFFull)
        return set_err(SA_E_INVALID, "%llu occurrences are more than 2^32 - 1: search fewer patterns a call",
                       (unsigned long long)total);
    if (own && total <= out_cap) {
        if (own->want_pos) {
            SA_TRY(own->pos.alloc(align_up(total, 64) * 4));
            d_pos = own->pos.as<uint32_t>();
        }
        if (own->want_dist) {
            SA_TRY(own->dist.alloc(align_up(total, 256)));
            d_dist = own->dist.as<uint8_t>();
        }
    }
    const bool write = d_pos != nullptr && total <= out_cap;
    LocBuf surv;   // the starts of the kept candidates, in candidate order
    if (write) SA_TRY(surv.alloc(align_up(total, 4) * 4, s));
    hipLaunchKernelGGL(k_ham_emit, dim3(list.grid), dim3(kBlock), 0, s, in, kk, (const uint64_t*)list.coff, np,
                       (const uint32_t*)list.cand, list.cands, (const uint8_t*)list.flagb, (const int64_t*)list.tcnt,
                       (uint32_t*)surv.p, d_lo2, d_hi2);
    SA_HIP(hipGetLastError());
    // the sizing call: the counts alone, from lo2 / hi2 (nothing is gathered, the candidates stand in)
    SA_TRY(sort_lists(c, "hamming", "occurrences", total, write ? (const uint32_t*)surv.p : list.cand, d_lo2, d_hi2, nq,
                      0, d_off, write ? d_pos : nullptr, out_cap, n, s));
    if (write && d_dist) {
        const uint64_t otiles = (total + kMemTile - 1) / kMemTile;
        const uint32_t ogrid = (uint32_t)std::min<uint64_t>(otiles, (uint64_t)c->cus * kMemGridPerCu);
        hipLaunchKernelGGL(k_ham_dist, dim3(ogrid), dim3(kBlock), 0, s, in, (const uint64_t*)d_off, nq,
                           (const uint32_t*)d_pos, total, lane_bytes, d_dist);
        SA_HIP(hipGetLastError());
        SA_HIP(host_sync(s));
    }
    return SA_OK;
}

// host in, host out (sa_hamming), over the steps of sa_host.h.  The device
// form finds the total; the outputs are allocated then.
static int hamming_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat,
                        const uint64_t* pat_off, uint64_t nq, uint64_t k, uint64_t max_candidates, uint32_t flags,
                        uint64_t* off_out, void* pos_out, uint8_t* dist_out, uint64_t out_cap, uint64_t* info) {
    SA_TRY(check_width(sa_width));
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (!off_out) return set_err(SA_E_INVALID, "off_out is NULL");
    SA_TRY(check_n32(n));
    SA_TRY(ham_check_sizes(nq, k));
    if (n && !text) return set_err(SA_E_INVALID, "text is NULL");
    if (n && !sa) return set_err(SA_E_INVALID, "sa is NULL");
    if (nq && !pat_off) return set_err(SA_E_INVALID, "pat_off is NULL");
    SA_TRY(ham_check_flags(flags));
    if (dist_out && !pos_out) return set_err(SA_E_INVALID, "dist_out without pos_out");
    for (uint64_t q = 0; q < nq; ++q)
        if (pat_off[q] > pat_off[q + 1])
            return set_err(SA_E_INVALID, "pattern offsets decrease at %llu", (unsigned long long)q);
    const uint64_t pat_bytes = nq ? pat_off[nq] : 0;
    if (pat_bytes && !pat) return set_err(SA_E_INVALID, "pat is NULL");
    SA_TRY(check_no_alias({off_out, pos_out, dist_out}, {text, sa, pat, pat_off}));
    SA_TRY(check_distinct({off_out, pos_out, dist_out}));
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    info[0] = info[1] = 0;
    info[2] = nq * (k + 1);
    if (nq == 0 || n == 0) {
        std::memset(off_out, 0, (nq + 1) * 8);
        return SA_OK;
    }
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_text, d_sa, d_pat, d_poff, d_off;
    HamOwn own;
    own.want_pos = pos_out != nullptr;
    own.want_dist = dist_out != nullptr;
    SA_TRY(d_text.alloc(align_up(n + 1, 256)));
    SA_TRY(d_sa.alloc(align_up(n + 1, 64) * 4));
    SA_TRY(d_pat.alloc(align_up(pat_bytes + 1, 256)));
    SA_TRY(d_poff.alloc((nq + 1) * 8));
    SA_TRY(d_off.alloc(align_up(nq + 1, 64) * 8));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}, {d_pat.p, pat, pat_bytes}, {d_poff.p, pat_off, (nq + 1) * 8}}));
    const int rc = hamming_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_pat.as<uint8_t>(), pat_bytes,
                                  d_poff.as<uint64_t>(), nq, k, max_candidates, flags, d_off.as<uint64_t>(), nullptr,
                                  nullptr, out_cap, info, nullptr, &own);
    if (rc < 0) return rc;
    SA_HIP(hipMemcpyAsync(off_out, d_off.p, (nq + 1) * 8, hipMemcpyDeviceToHost, nullptr));
    SA_HIP(host_sync(nullptr));
    if (rc == SA_OK && own.pos.p) {
        SA_TRY(copy_d2h(pos_out, own.pos.as<uint32_t>(), info[0], sa_width, nullptr));
        if (own.dist.p) {
            SA_HIP(hipMemcpyAsync(dist_out, own.dist.p, info[0], hipMemcpyDeviceToHost, nullptr));
            SA_HIP(host_sync(nullptr));
        }
    }
    return rc;
}

}  // namespace sa

extern "C" {

int sa_hamming_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                      uint64_t pat_bytes, const uint64_t* d_pat_off, uint64_t nq, uint64_t k, uint64_t max_candidates,
                      uint32_t flags, uint64_t* d_off, uint32_t* d_pos, uint8_t* d_dist, uint64_t out_cap,
                      uint64_t info[SA_HAMMING_INFO], void* stream) {
    return sa::hamming_device(ctx, d_text, n, d_sa, d_pat, pat_bytes, d_pat_off, nq, k, max_candidates, flags, d_off,
                              d_pos, d_dist, out_cap, info, (hipStream_t)stream);
}

int sa_hamming(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat, const uint64_t* pat_off,
               uint64_t nq, uint64_t k, uint64_t max_candidates, uint32_t flags, uint64_t* off_out, void* pos_out,
               uint8_t* dist_out, uint64_t out_cap, uint64_t info[SA_HAMMING_INFO]) {
    return sa::hamming_host(text, n, sa, sa_width, pat, pat_off, nq, k, max_candidates, flags, off_out, pos_out, dist_out,
                            out_cap, info);
}

}  // extern "C"

#endif   // __HIPCC__
