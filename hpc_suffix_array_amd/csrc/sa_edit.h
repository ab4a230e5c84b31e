// sa_edit.h -- k-difference (edit distance) pattern search over a built suffix
// array (sa_edit / sa_edit_device of include/sa_hip.h).
//
// Definition.  Text T of n bytes, pattern P of m bytes, one budget k per call
// with 0 <= k <= SA_EDIT_MAX_K = 31.  For an end e in [0, n] let D(e) = min
// over s <= e of ed(P, T[s, e)), ed the unit-cost Levenshtein distance
// (Sellers).  An occurrence is an end e with D(e) <= k; its distance is D(e)
// and its start the largest s with ed(P, T[s, e)) = D(e), the shortest best
// match.  A pattern with m <= k matches at every end: it is not searched and
// its list is empty (its pieces are still counted in info[2]).  A pattern with
// m > n is searched.  Bytes are sa_find's: binary-safe, explicit lengths.
// Output: CSR over the queries: off (nq + 1 uint64, off[0] = 0), end (uint32,
// ascending inside a query, every end once), start (uint32) and dist (uint8) of
// the same slot, each may be NULL.
//
// Seeds.  The pieces are sa_hamming.h's: piece j = P[b_j, b_{j+1}) with b_j =
// floor(j m / (k + 1)), all non-empty because m >= k + 1.  An alignment with at
// most k edits leaves one piece untouched, so that piece occurs exactly at text
// position h with the alignment passing through (row b_j, column h): on the
// diagonal c = h - b_j (signed).  Every such alignment lies within the
// diagonals c - k .. c + k.
//
// The band.  Row i (i bytes of P consumed) holds the 2k + 1 <= 63 cells t of
// the columns x = i + c - k + t; cell t of row i + 1 lies diagonally below cell
// t of row i, its upper neighbour is cell t + 1 and its left one cell t - 1 of
// its own row.  The row is kept as the horizontal differences of neighbouring
// cells in two words (plus / minus one), and a row step is Myers' bit-vector
// step in Hyyro's banded form: the diagonal differences d0 come out of one
// addition, and the band slides by a shift of d0 instead of a shift of the row.
// What lies above the band's last cell is never smaller, what lies left of its
// first cell neither: the carry into bit 0 is 0 and the bits above the band are
// masked.  The equality word of a row is built by SWAR compares of the row's
// 2k + 1 text bytes against P[i] (edit_eq_window).  Columns outside [0, n] are
// handled without a second path: their text bytes match nothing.  To the right
// of n they cannot reach a column <= n; to the left of 0 a path over them costs
// no less than the path down column 0 that stays inside the band whenever a
// cell of row 0 has a column >= 0 (c + k >= 0; otherwise the band has no start
// and the answer is empty).  So the cells of the columns in [0, n] hold exactly
// D_band, the distance restricted to the band with a free start in row 0.
//
// A cell's value is the number of rows whose d0 bit was 0 (row 0 is 0), so
// "value > k" is kept per cell by bit-sliced counters that start at
// 2^NS - 1 - k and set a sticky bit on overflow (NS = 2 for k <= 3, 5
// otherwise).  When every cell is dead the candidate is dropped (Ukkonen's
// cut-off): in a random text that happens within a few rows.  The candidate's
// result is the mask of the cells alive in row m whose column is in [0, n]:
// bit t stands for the end c + m - k + t.
//
//   k_ham_pieces   the piece offsets (sa_hamming.h).
//   find_device    on the pieces: [lo, hi) per piece.
//   k_edit_seeds   empties the intervals of the patterns with m <= k and counts
//                  the candidates; the host reads the count (the first wait),
//                  applies max_candidates and sizes the list.
//   locate_device  with SA_LOCATE_SA_ORDER (CandList::fill).
//   k_edit_verify  the hot kernel: a lane per candidate over the tiles of
//                  sa_query.h, one 64-bit mask per candidate, a count per tile.
//                  While the tiles are fewer than an eighth of the grid a tile
//                  is shared by kMemPer workgroups, one candidate a lane.
//                  A candidate is dropped unseen when an earlier piece matches
//                  exactly on its diagonal: that piece's candidate computes the
//                  same band.
//   scan           over the tile counts; the host reads the total (a wait).
//   k_edit_emit    the ends of the masks in candidate order, each query's range.
//   sort_lists     into a temporary, ascending per query (its limits are
//                  inherited: at most 2^32 - 1 ends before the unique).
//   k_edit_uniq_flag, scan, k_edit_uniq_emit   the first of each run of equal
//                  ends of a query; the emit also writes the final off.  The
//                  host reads the total in between (a wait).
//   k_edit_finish  when start or dist is wanted: per end e the anchored DP
//                  backwards, A[i][x] = ed(P[m - i, m), T[e - x, e)) within
//                  |x - i| <= k, x <= e, A[0][x] = x; D(e) is the least A[m][x]
//                  and the start e - (the smallest such x).  The same row step,
//                  the equality word bit-reversed.
// The sizing call (end NULL or the total above out_cap) does all of this but
// k_edit_finish, and writes off and info.
//
// The host-compilable core comes first (tests/cpp/edit_check.cpp checks it
// against the full DP); the HIP part needs sa_hamming.h before it.
// Measurements and the resource report: DESIGN.md section 23.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "sa_hamming.h"   // ham_piece_bound, ham_count_lane

// full unrolling keeps the counter slices in registers; g++ (the host check) has no such pragma
#if defined(__clang__)
#define SA_EDIT_UNROLL _Pragma("unroll")
#else
#define SA_EDIT_UNROLL
#endif

namespace sa {

// the largest budget (= SA_EDIT_MAX_K): the band of 2k + 1 cells fits a word
constexpr uint32_t kEditMaxK = 31;

// the low c bits
SA_HD uint64_t edit_low_bits(uint64_t c) { return c >= 64 ? ~0ull : (1ull << c) - 1ull; }

SA_HD uint64_t edit_reverse64(uint64_t x) {
#if defined(__clang__)
    return __builtin_bitreverse64(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
#endif
}

// bit j of the result: byte j of w equals b
SA_HD uint64_t edit_eq_bytes(uint64_t w, uint8_t b) {
    const uint64_t lo7 = 0x7F7F7F7F7F7F7F7Full;
    const uint64_t x = w ^ ((uint64_t)b * 0x0101010101010101ull);
    const uint64_t z = ~(((x & lo7) + lo7) | x | lo7);   // 0x80 in the zero bytes of x
    return ((z >> 7) * 0x0102040810204080ull) >> 56;     // no two partial products share a bit
}

// bit u (u < width <= 64) of the result: T[tau0 + u] == b, and 0 <= tau0 + u <
// limit.  text_word(x), 0 <= x < limit: the little-endian 8 bytes at text
// position x, zero past the end of the text; limit <= n.
template <class TextWord>
SA_HD uint64_t edit_eq_window(const TextWord& text_word, int64_t limit, int64_t tau0, uint32_t width, uint8_t b) {
    if (limit <= 0 || tau0 >= limit || tau0 + (int64_t)width <= 0) return 0;
    uint64_t eq = 0;
    for (uint32_t w = 0; w < width; w += 8) {
        const int64_t tau = tau0 + (int64_t)w;
        if (tau >= limit) break;
        if (tau + 8 <= 0) continue;
        const uint64_t word = tau >= 0 ? text_word((uint64_t)tau) : text_word(0) << (8 * (uint32_t)(-tau));
        eq |= edit_eq_bytes(word, b) << w;
    }
    const uint64_t cut = tau0 < 0 ? edit_low_bits((uint64_t)(-tau0)) : 0ull;
    return eq & edit_low_bits((uint64_t)std::min<int64_t>(limit - tau0, (int64_t)width)) & ~cut;
}

// One row of the band.  ap / an: bit t is set when cell t + 1 is one more / one
// less than cell t (bit 2k: towards the cell above the band, never minus).
// Returns d0: bit t is set when cell t of the new row equals cell t of the old.
SA_HD uint64_t edit_step(uint64_t eq, uint64_t band, uint64_t& ap, uint64_t& an) {
    const uint64_t d0 = ((((eq & ap) + ap) ^ ap) | eq | an) & band;
    const uint64_t vp = an | ~(d0 | ap), vn = d0 & ap;   // the new cell t against the old cell t + 1
    const uint64_t x = d0 >> 1;
    an = x & vp;
    ap = (vn | ~(x | vp)) & band;
    return d0;
}

// The band of the diagonals c - k .. c + k with a free start in row 0: bit t
// of the result is set iff D_band[m][c + m - k + t] <= k and that column is in
// [0, n].  NS: counter slices, 2^NS >= k + 1.  pat_word(x), x < m: 8 bytes of
// the pattern.  m >= 1.
template <int NS, class TextWord, class PatWord>
SA_HD uint64_t edit_verify_band(uint64_t n, uint64_t m, uint32_t k, int64_t c, const TextWord& text_word,
                                const PatWord& pat_word) {
    const uint32_t width = 2 * k + 1;
    const uint64_t band = edit_low_bits(width);
    const int64_t base = c - (int64_t)k, e0 = base + (int64_t)m;   // the column of bit 0 in row 0 / row m
    if (c + (int64_t)k < 0 || e0 > (int64_t)n) return 0;
    uint64_t ap = 0, an = 0, dead = 0, cnt[NS], pw = 0;
SA_EDIT_UNROLL
    for (int s = 0; s < NS; ++s) cnt[s] = ((((1u << NS) - 1u - k) >> s) & 1u) ? band : 0ull;
    for (uint64_t i = 0; i < m; ++i) {
        if ((i & 7) == 0) pw = pat_word(i);
        const uint64_t eq = edit_eq_window(text_word, (int64_t)n, base + (int64_t)i, width, (uint8_t)pw);
        pw >>= 8;
        uint64_t carry = ~edit_step(eq, band, ap, an) & band;   // the cells that grew
SA_EDIT_UNROLL
        for (int s = 0; s < NS; ++s) {
            const uint64_t t = cnt[s] & carry;
            cnt[s] ^= carry;
            carry = t;
        }
        dead |= carry;
        if (dead == band) return 0;
    }
    const uint64_t cut = e0 < 0 ? edit_low_bits((uint64_t)(-e0)) : 0ull;
    return ~dead & band & edit_low_bits((uint64_t)((int64_t)n - e0) + 1u) & ~cut;
}

// the band of candidate (piece j, hit h) of a pattern of m > k bytes; 0 for a
// hit >= n (an invalid SA) and when an earlier piece matches exactly on the
// same diagonal (its candidate computes this band)
template <class TextWord, class PatWord>
SA_HD uint64_t edit_candidate_mask(uint64_t n, uint64_t m, uint32_t k, uint32_t j, uint64_t h, const TextWord& text_word,
                                   const PatWord& pat_word) {
    if (h >= n || m <= k) return 0;
    const int64_t c = (int64_t)h - (int64_t)ham_piece_bound(m, k, j);
    if (c >= 0) {
        uint64_t b = 0;
        for (uint32_t jj = 0; jj < j; ++jj) {
            const uint64_t e = ham_piece_bound(m, k, jj + 1);
            if ((uint64_t)c + e <= n && ham_count_lane((uint64_t)c, b, e, 0, text_word, pat_word) == 0) return 0;
            b = e;
        }
    }
    return k <= 3 ? edit_verify_band<2>(n, m, k, c, text_word, pat_word)
                  : edit_verify_band<5>(n, m, k, c, text_word, pat_word);
}

// the end that bit t of a candidate's mask stands for (in [0, n] for a set bit)
SA_HD uint64_t edit_mask_end(uint64_t m, uint32_t k, uint32_t j, uint64_t h, uint32_t t) {
    return (uint64_t)((int64_t)h - (int64_t)ham_piece_bound(m, k, j) + (int64_t)m - (int64_t)k + (int64_t)t);
}

// Distance and start of the end e <= n of a pattern of m > k bytes, exact when
// D(e) <= k.  Cell t of row i is the column x = i - k + t of the anchored DP
// over P and T[0, e) reversed; row 0 is |x|, which gives the columns below 0
// no path cheaper than the one down column 0.  false: no column of row m is in
// [0, e] (not an occurrence).
template <class TextWord, class PatWord>
SA_HD bool edit_finish_end(uint64_t m, uint32_t k, uint64_t e, const TextWord& text_word, const PatWord& pat_word,
                           uint64_t& start, uint32_t& dist) {
    const uint32_t width = 2 * k + 1;
    const uint64_t band = edit_low_bits(width);
    uint64_t an = edit_low_bits(k), ap = band & ~an, s0 = k, pw = 0;   // s0: cell 0
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t at = m - 1 - i;   // the pattern byte of this row
        if (i == 0 || (at & 7) == 7) pw = pat_word(at & ~7ull);
        const uint8_t b = (uint8_t)(pw >> (8 * (at & 7)));
        // cell t of the new row compares T[e - x], x = i + 1 - k + t: the window in text order, then reversed
        const uint64_t eqf = edit_eq_window(text_word, (int64_t)e, (int64_t)e - 1 - (int64_t)i - (int64_t)k, width, b);
        const uint64_t d0 = edit_step(edit_reverse64(eqf) >> (64 - width), band, ap, an);
        s0 += 1u - (d0 & 1u);
    }
    uint64_t best = ~0ull, val = s0, bx = 0;
    for (uint32_t t = 0; t < width; ++t) {
        const uint64_t x = m - k + t;   // >= 1
        if (x <= e && val < best) {
            best = val;
            bx = x;
        }
        val = val + ((ap >> t) & 1u) - ((an >> t) & 1u);
    }
    if (best == ~0ull) return false;
    start = e - bx;
    dist = (uint32_t)std::min<uint64_t>(best, 255);
    return true;
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

namespace sa {

static_assert(SA_EDIT_MAX_K == 31 && SA_EDIT_INFO == 3 && SA_EDIT_TOO_MANY == 1, "sa_hip.h states these");
static_assert(kEditMaxK == SA_EDIT_MAX_K && 2 * kEditMaxK + 1 <= 63, "the header's largest budget; the band in a word");
static_assert(kBlock % 8 == 0, "CandList::extra holds 64-bit masks");

// lo = hi = 0 for the pieces of the patterns with m <= k; word[0] += the hits of the others
__global__ __launch_bounds__(kBlock) void k_edit_seeds(const uint64_t* __restrict__ pat_off, uint64_t pat_bytes, uint32_t k,
                                                       uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint64_t np,
                                                       uint64_t n, unsigned long long* __restrict__ word) {
    const uint64_t k1 = (uint64_t)k + 1u;
    unsigned long long c[1] = {0};
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < np; g += (uint64_t)gridDim.x * kBlock) {
        uint64_t a, m;
        find_pattern(pat_off, g / k1, pat_bytes, a, m);
        if (m <= k) lo[g] = hi[g] = 0u;
        else c[0] += locate_count(lo[g], hi[g], n, 0);
    }
    block_sum_u64(c, word);
}

// mask[x]: the band of candidate x (edit_candidate_mask); tcnt[t]: the set bits of tile t.  parts = 1: a
// workgroup takes whole tiles, kMemPer candidates a lane.  parts = kMemPer (the host's choice while the tiles
// alone would leave workgroups idle): a tile is shared by kMemPer workgroups, a candidate a lane, and tcnt,
// zeroed by the host, takes their sums by one atomic each (integers: the same sum in any order).
__global__ __launch_bounds__(kBlock) void k_edit_verify(HamIn in, uint32_t k, const uint64_t* __restrict__ coff,
                                                        uint64_t np, const uint32_t* __restrict__ cand, uint64_t total,
                                                        uint32_t parts, uint64_t* __restrict__ mask,
                                                        int64_t* __restrict__ tcnt) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t k1 = k + 1u;
    const uint64_t work = (total + kMemTile - 1) / kMemTile * parts;
    for (uint64_t w = blockIdx.x; w < work; w += gridDim.x) {
        const uint64_t t = w / parts;
        const uint32_t part = (uint32_t)(w - t * parts);
        uint32_t pos[kMemPer];
        const MemTile r = mem_tile_positions(coff, np, t, total, s_pos, s_w, s_q, pos);
        // one body for the lane's candidates (the DP is not unrolled kMemPer times), their pieces from s_pos;
        // neighbouring lanes take neighbouring candidates: the same piece, rows of the same length
        uint32_t ends = 0;
#pragma unroll 1
        for (uint32_t slot = part * kBlock + tid; slot < r.cnt; slot += parts * kBlock) {
            const uint32_t g = s_pos[slot], q = g / k1;
            uint64_t pa, m;
            find_pattern(in.pat_off, q, in.pat_bytes, pa, m);
            const uint64_t mk = edit_candidate_mask(
                in.n, m, k, g - q * k1, cand[r.s + slot], [&](uint64_t x) { return load8(in.text, x, in.n); },
                [&](uint64_t x) { return load8(in.pat, pa + x, in.pat_bytes); });
            mask[r.s + slot] = mk;
            ends += (uint32_t)__builtin_popcountll(mk);
        }
        uint32_t sum;
        (void)mem_block_excl(ends, s_w, sum);   // its barriers: s_pos is free for the next tile
        if (tid == 0) {
            if (parts == 1) tcnt[t] = (int64_t)sum;
            else if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(tcnt + t), (unsigned long long)sum);
        }
    }
}

// tbase: the inclusive sums of the tile counts.  ends takes the ends of the
// masks in candidate order, a candidate's ascending; lo2 / hi2 take each
// query's range in it, from the ranks at the piece boundaries q (k + 1).
__global__ __launch_bounds__(kBlock) void k_edit_emit(HamIn in, uint32_t k, const uint64_t* __restrict__ coff, uint64_t np,
                                                      const uint32_t* __restrict__ cand, uint64_t total,
                                                      const uint64_t* __restrict__ mask,
                                                      const int64_t* __restrict__ tbase, uint32_t* __restrict__ ends,
                                                      uint32_t* __restrict__ lo2, uint32_t* __restrict__ hi2) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint32_t s_rank[kMemTile + 1];   // ends of the tile in front of each slot; [kMemTile]: all
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t k1 = k + 1u;
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t pos[kMemPer];
        const MemTile r = mem_tile_positions(coff, np, t, total, s_pos, s_w, s_q, pos);
        const uint64_t base = t ? (uint64_t)tbase[t - 1] : 0;
        uint64_t mk[kMemPer];
        uint32_t mine_cnt = 0;
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            const uint32_t slot = kMemPer * tid + j;
            mk[j] = slot < r.cnt ? mask[r.s + slot] : 0ull;
            mine_cnt += (uint32_t)__builtin_popcountll(mk[j]);
        }
        uint32_t sum;
        uint32_t rank = mem_block_excl(mine_cnt, s_w, sum);
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            s_rank[kMemPer * tid + j] = rank;
            rank += (uint32_t)__builtin_popcountll(mk[j]);
        }
        if (tid == 0) s_rank[kMemTile] = sum;
        __syncthreads();
        // the pieces whose list starts here (masks past cnt are 0, so s_rank[cnt] is the tile's sum); the last
        // tile takes those at the very end and the end of the last query
        const uint64_t g_end = t + 1 == tiles ? np + 1 : r.q_hi;
        for (uint64_t g = r.q_lo + tid; g < g_end; g += kBlock) {
            const uint64_t q = g / k1;
            if (g != q * k1) continue;
            const uint64_t a = coff[g];
            const uint32_t slot = a >= r.s ? (uint32_t)std::min<uint64_t>(a - r.s, r.cnt) : 0u;
            const uint32_t at = (uint32_t)(base + s_rank[slot]);   // the host stops above 2^32 - 1 ends
            if (g < np) lo2[q] = at;
            if (q > 0) hi2[q - 1] = at;
        }
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            uint64_t bits = mk[j];
            if (!bits) continue;
            const uint32_t slot = kMemPer * tid + j;
            const uint32_t g = pos[j], q = g / k1;
            uint64_t pa, m;
            find_pattern(in.pat_off, q, in.pat_bytes, pa, m);
            const uint32_t hit = cand[r.s + slot];
            uint64_t at = base + s_rank[slot];
            while (bits) {
                const uint32_t b = (uint32_t)__builtin_ctzll(bits);
                bits &= bits - 1ull;
                ends[at++] = (uint32_t)edit_mask_end(m, k, g - q * k1, hit, b);   // <= n
            }
        }
        __syncthreads();   // the next tile writes these arrays
    }
}

// flagb[t * kBlock + lane of the workgroup]: bit j = sorted end t * kMemTile + kMemPer * lane + j is the first
// of its run inside its query; tcnt[t]: the tile's count.  toff: the nq + 1 offsets of the sorted lists.
__global__ __launch_bounds__(kBlock) void k_edit_uniq_flag(const uint64_t* __restrict__ toff, uint64_t nq,
                                                           const uint32_t* __restrict__ sorted, uint64_t total,
                                                           uint8_t* __restrict__ flagb, int64_t* __restrict__ tcnt) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t own[kMemPer];
        const MemTile r = mem_tile_positions(toff, nq, t, total, s_pos, s_w, s_q, own);
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < kMemPer; ++j) {
            const uint32_t slot = kMemPer * tid + j;
            if (slot >= r.cnt) continue;
            const uint64_t x = r.s + slot;
            if (x == 0 || x == toff[own[j]] || sorted[x] != sorted[x - 1]) bits |= 1u << j;
        }
        uint32_t sum;
        (void)mem_block_excl((uint32_t)__popc(bits), s_w, sum);
        flagb[t * kBlock + tid] = (uint8_t)bits;
        if (tid == 0) tcnt[t] = (int64_t)sum;
    }
}

// off[q]: the flagged ends in front of query q's list (off[nq]: all of them); end (may be NULL: the sizing
// call) takes the flagged ends in order
__global__ __launch_bounds__(kBlock) void k_edit_uniq_emit(const uint64_t* __restrict__ toff, uint64_t nq,
                                                           const uint32_t* __restrict__ sorted, uint64_t total,
                                                           const uint8_t* __restrict__ flagb,
                                                           const int64_t* __restrict__ tbase, uint64_t* __restrict__ off,
                                                           uint32_t* __restrict__ end) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kMemTile];
    __shared__ uint32_t s_rank[kMemTile + 1];
    __shared__ uint32_t s_w[kWaves];
    __shared__ uint64_t s_q[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = (total + kMemTile - 1) / kMemTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t own[kMemPer];
        const MemTile r = mem_tile_positions(toff, nq, t, total, s_pos, s_w, s_q, own);
        const uint64_t base = t ? (uint64_t)tbase[t - 1] : 0;
        uint32_t bits = flagb[t * kBlock + tid];
        uint32_t sum;
        const uint32_t mine = mem_block_excl((uint32_t)__popc(bits), s_w, sum);
#pragma unroll
        for (int j = 0; j < kMemPer; ++j)
            s_rank[kMemPer * tid + j] = mine + (uint32_t)__popc(bits & ((1u << j) - 1u));
        if (tid == 0) s_rank[kMemTile] = sum;
        __syncthreads();
        const uint64_t g_end = t + 1 == tiles ? nq + 1 : r.q_hi;
        for (uint64_t g = r.q_lo + tid; g < g_end; g += kBlock) {
            const uint64_t a = toff[g];
            const uint32_t slot = a >= r.s ? (uint32_t)std::min<uint64_t>(a - r.s, r.cnt) : 0u;
            off[g] = base + s_rank[slot];
        }
        if (end) {
            while (bits) {
                const int j = __builtin_ctz(bits);
                bits &= bits - 1u;
                const uint32_t slot = kMemPer * tid + j;
                end[base + s_rank[slot]] = sorted[r.s + slot];
            }
        }
        __syncthreads();   // the next tile writes these arrays
    }
}

// start[x] / dist[x] (each may be NULL) of the `total` ends in output order, a lane per end; off: the nq + 1
// offsets of the output
__global__ __launch_bounds__(kBlock) void k_edit_finish(HamIn in, uint32_t k, const uint64_t* __restrict__ off,
                                                        uint64_t nq, const uint32_t* __restrict__ end, uint64_t total,
                                                        uint32_t* __restrict__ start, uint8_t* __restrict__ dist) {
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < total; x += (uint64_t)gridDim.x * kBlock) {
        // the last query whose list begins at or in front of x (off[nq] = total > x)
        const uint64_t q = locate_lower_bound(LocOff{off}, 0, nq + 1, x + 1) - 1;
        uint64_t pa, m;
        find_pattern(in.pat_off, q, in.pat_bytes, pa, m);
        const uint64_t e = end[x];
        uint64_t s = e;
        uint32_t d = 255u;
        if (e <= in.n && m > k)   // an occurrence; anything else reads nothing
            (void)edit_finish_end(m, k, e, [&](uint64_t y) { return load8(in.text, y, in.n); },
                                  [&](uint64_t y) { return load8(in.pat, pa + y, in.pat_bytes); }, s, d);
        if (start) start[x] = (uint32_t)s;
        if (dist) dist[x] = (uint8_t)d;
    }
}

static int edit_check_sizes(uint64_t nq, uint64_t k) {
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (k > SA_EDIT_MAX_K) return set_err(SA_E_INVALID, "k is above SA_EDIT_MAX_K = %d", SA_EDIT_MAX_K);
    if (nq * (k + 1) > 0xFFFFFFFFull)
        return set_err(SA_E_INVALID, "nq (k + 1) = %llu pieces are more than 2^32 - 1", (unsigned long long)(nq * (k + 1)));
    return SA_OK;
}

// the checks of sa_edit_device, all before any HIP call
static int edit_check_args(const sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                           const uint8_t* d_pat, uint64_t pat_bytes, const uint64_t* d_pat_off, uint64_t nq, uint64_t k,
                           uint32_t flags, const uint64_t* d_off, const uint32_t* d_end, const uint32_t* d_start,
                           const uint8_t* d_dist, const uint64_t* info) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (!d_off) return set_err(SA_E_INVALID, "d_off is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    SA_TRY(edit_check_sizes(nq, k));
    if (n && !d_text) return set_err(SA_E_INVALID, "d_text is NULL");
    if (n && !d_sa) return set_err(SA_E_INVALID, "d_sa is NULL");
    if (pat_bytes && !d_pat) return set_err(SA_E_INVALID, "d_pat is NULL");
    if (nq && !d_pat_off) return set_err(SA_E_INVALID, "d_pat_off is NULL");
    SA_TRY(check_flags(flags, 0u));
    if (d_start && !d_end) return set_err(SA_E_INVALID, "d_start without d_end");
    if (d_dist && !d_end) return set_err(SA_E_INVALID, "d_dist without d_end");
    SA_TRY(check_no_alias({d_off, d_end, d_start, d_dist}, {d_text, d_sa, d_pat, d_pat_off}));
    return check_distinct({d_off, d_end, d_start, d_dist});
}

// the host form's outputs, allocated when the total is known
struct EditOwn {
    DevBuf end, start, dist;
    bool want_end = false, want_start = false, want_dist = false;   // the caller gave host outputs
};

// Host waits: the candidate count; locate_device's own over the pieces (one, two when a piece has more than
// SA_LOCATE_TILE hits); the ends before the unique; locate_device_n's own over them (one, more when a query
// has more than SA_LOCATE_TILE of them); the total; one at the end.
static int edit_device(sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                       uint64_t pat_bytes, const uint64_t* d_pat_off, uint64_t nq, uint64_t k, uint64_t max_candidates,
                       uint32_t flags, uint64_t* d_off, uint32_t* d_end, uint32_t* d_start, uint8_t* d_dist,
                       uint64_t out_cap, uint64_t* info, hipStream_t s, EditOwn* own = nullptr) {
    SA_TRY(edit_check_args(c, d_text, n, d_sa, d_pat, pat_bytes, d_pat_off, nq, k, flags, d_off, d_end, d_start, d_dist,
                           info));
    const uint64_t np = nq * (k + 1);
    info[0] = info[1] = 0;
    info[2] = np;
    SA_HIP(hipSetDevice(c->device));
    if (nq == 0 || n == 0) return empty_csr(d_off, nq, s);
    uint64_t* h = host_u64<kHwEdit, 3>(c);
    // no byte of an empty buffer is read (load8 ends at pat_bytes): any pointer serves
    const HamIn in{d_text, n, d_pat ? d_pat : d_text, pat_bytes, d_pat_off};
    const uint32_t kk = (uint32_t)k;
    const uint32_t pgrid = (uint32_t)std::min<uint64_t>((np + kBlock) / kBlock, (uint64_t)c->cus * 8);
    CandList list;   // extra: the masks | lo2 | hi2
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
        hipLaunchKernelGGL(k_edit_seeds, dim3(pgrid), dim3(kBlock), 0, s, d_pat_off, pat_bytes, kk, d_lo, d_hi, np, n,
                           d_word);
        SA_HIP(hipGetLastError());
        SA_HIP(hipMemcpyAsync(h, d_word, 8, hipMemcpyDeviceToHost, s));
        SA_HIP(host_sync(s));
        info[1] = h[0];
        SA_TRACE("edit: nq %llu k %u pieces %llu candidates %llu", (unsigned long long)nq, kk, (unsigned long long)np,
                 (unsigned long long)h[0]);
        const int rc = list.fill(c, "edit", n, d_sa, d_lo, d_hi, np, h[0], max_candidates, SA_EDIT_TOO_MANY, d_off, nq,
                                 SA_LOCATE_SA_ORDER, h[0] * 8 + 2 * nq * 4, s);
        if (rc || !list.tiles) return rc;
    }
    uint64_t* d_mask = (uint64_t*)list.extra;
    uint32_t *d_lo2 = (uint32_t*)(d_mask + list.cands), *d_hi2 = d_lo2 + nq;
    // few tiles: a candidate a lane over kMemPer times the workgroups (a long pattern's band is thousands of rows)
    const uint32_t parts = list.tiles * kMemPer <= (uint64_t)c->cus * kMemGridPerCu ? (uint32_t)kMemPer : 1u;
    if (parts > 1) SA_HIP(hipMemsetAsync(list.tcnt, 0, list.tiles * 8, s));
    hipLaunchKernelGGL(k_edit_verify, dim3(parts > 1 ? (uint32_t)(list.tiles * parts) : list.grid), dim3(kBlock), 0, s,
                       in, kk, (const uint64_t*)list.coff, np, (const uint32_t*)list.cand, list.cands, parts, d_mask,
                       list.tcnt);
    SA_HIP(hipGetLastError());
    SA_TRY(list.scan(s));
    uint64_t pre = 0;   // the ends before the unique
    SA_TRY(list.total(h + 1, s, &pre));
    if (pre == 0) return empty_csr(d_off, nq, s);
    if (pre > 0xFFFFFFFFull)
        return set_err(SA_E_INVALID, "%llu ends before the unique are more than 2^32 - 1: search fewer patterns a call",
                       (unsigned long long)pre);
    const uint64_t utiles = (pre + kMemTile - 1) / kMemTile;
    const uint32_t ugrid = (uint32_t)std::min<uint64_t>(utiles, (uint64_t)c->cus * kMemGridPerCu);
    LocBuf u;   // the sorted lists' offsets (nq + 1) | tile counts | the ends in candidate order | sorted | flag bytes
    SA_TRY(u.alloc((nq + 1) * 8 + utiles * 8 + 2 * align_up(pre, 4) * 4 + utiles * kBlock, s));
    uint64_t* d_toff = (uint64_t*)u.p;
    int64_t* d_ucnt = (int64_t*)(d_toff + nq + 1);
    uint32_t* d_raw = (uint32_t*)(d_ucnt + utiles);
    uint32_t* d_sorted = d_raw + align_up(pre, 4);
    uint8_t* d_uflag = (uint8_t*)(d_sorted + align_up(pre, 4));
    hipLaunchKernelGGL(k_edit_emit, dim3(list.grid), dim3(kBlock), 0, s, in, kk, (const uint64_t*)list.coff, np,
                       (const uint32_t*)list.cand, list.cands, (const uint64_t*)d_mask, (const int64_t*)list.tcnt, d_raw,
                       d_lo2, d_hi2);
    SA_HIP(hipGetLastError());
    // an end is a position of [0, n]
    SA_TRY(sort_lists(c, "edit", "ends", pre, d_raw, d_lo2, d_hi2, nq, 0, d_toff, d_sorted, pre, n + 1, s));
    hipLaunchKernelGGL(k_edit_uniq_flag, dim3(ugrid), dim3(kBlock), 0, s, (const uint64_t*)d_toff, nq,
                       (const uint32_t*)d_sorted, pre, d_uflag, d_ucnt);
    SA_HIP(hipGetLastError());
    SA_TRY(scan_i64<ScanSum>(d_ucnt, utiles, s));
    SA_HIP(hipMemcpyAsync(h + 2, d_ucnt + (utiles - 1), 8, hipMemcpyDeviceToHost, s));
    SA_HIP(host_sync(s));
    const uint64_t total = info[0] = h[2];
    if (own && total <= out_cap) {
        if (own->want_end) {
            SA_TRY(own->end.alloc(align_up(total, 64) * 4));
            d_end = own->end.as<uint32_t>();
        }
        if (own->want_start) {
            SA_TRY(own->start.alloc(align_up(total, 64) * 4));
            d_start = own->start.as<uint32_t>();
        }
        if (own->want_dist) {
            SA_TRY(own->dist.alloc(align_up(total, 256)));
            d_dist = own->dist.as<uint8_t>();
        }
    }
    const bool write = d_end != nullptr && total <= out_cap;
    hipLaunchKernelGGL(k_edit_uniq_emit, dim3(ugrid), dim3(kBlock), 0, s, (const uint64_t*)d_toff, nq,
                       (const uint32_t*)d_sorted, pre, (const uint8_t*)d_uflag, (const int64_t*)d_ucnt, d_off,
                       write ? d_end : nullptr);
    SA_HIP(hipGetLastError());
    if (write && (d_start || d_dist)) {
        const uint32_t fgrid = (uint32_t)std::min<uint64_t>((total + kBlock - 1) / kBlock, (uint64_t)c->cus * 8);
        hipLaunchKernelGGL(k_edit_finish, dim3(fgrid), dim3(kBlock), 0, s, in, kk, (const uint64_t*)d_off, nq,
                           (const uint32_t*)d_end, total, d_start, d_dist);
        SA_HIP(hipGetLastError());
    }
    SA_HIP(host_sync(s));
    return SA_OK;
}

// host in, host out (sa_edit), over the steps of sa_host.h.  The device form finds the total; the outputs
// are allocated then.
static int edit_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat,
                     const uint64_t* pat_off, uint64_t nq, uint64_t k, uint64_t max_candidates, uint32_t flags,
                     uint64_t* off_out, void* end_out, void* start_out, uint8_t* dist_out, uint64_t out_cap,
                     uint64_t* info) {
    SA_TRY(check_width(sa_width));
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (!off_out) return set_err(SA_E_INVALID, "off_out is NULL");
    SA_TRY(check_n32(n));
    SA_TRY(edit_check_sizes(nq, k));
    if (n && !text) return set_err(SA_E_INVALID, "text is NULL");
    if (n && !sa) return set_err(SA_E_INVALID, "sa is NULL");
    if (nq && !pat_off) return set_err(SA_E_INVALID, "pat_off is NULL");
    SA_TRY(check_flags(flags, 0u));
    if (start_out && !end_out) return set_err(SA_E_INVALID, "start_out without end_out");
    if (dist_out && !end_out) return set_err(SA_E_INVALID, "dist_out without end_out");
    for (uint64_t q = 0; q < nq; ++q)
        if (pat_off[q] > pat_off[q + 1])
            return set_err(SA_E_INVALID, "pattern offsets decrease at %llu", (unsigned long long)q);
    const uint64_t pat_bytes = nq ? pat_off[nq] : 0;
    if (pat_bytes && !pat) return set_err(SA_E_INVALID, "pat is NULL");
    SA_TRY(check_no_alias({off_out, end_out, start_out, dist_out}, {text, sa, pat, pat_off}));
    SA_TRY(check_distinct({off_out, end_out, start_out, dist_out}));
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
    EditOwn own;
    own.want_end = end_out != nullptr;
    own.want_start = start_out != nullptr;
    own.want_dist = dist_out != nullptr;
    SA_TRY(d_text.alloc(align_up(n + 1, 256)));
    SA_TRY(d_sa.alloc(align_up(n + 1, 64) * 4));
    SA_TRY(d_pat.alloc(align_up(pat_bytes + 1, 256)));
    SA_TRY(d_poff.alloc((nq + 1) * 8));
    SA_TRY(d_off.alloc(align_up(nq + 1, 64) * 8));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}, {d_pat.p, pat, pat_bytes}, {d_poff.p, pat_off, (nq + 1) * 8}}));
    const int rc = edit_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_pat.as<uint8_t>(), pat_bytes,
                               d_poff.as<uint64_t>(), nq, k, max_candidates, flags, d_off.as<uint64_t>(), nullptr, nullptr,
                               nullptr, out_cap, info, nullptr, &own);
    if (rc < 0) return rc;
    SA_HIP(hipMemcpyAsync(off_out, d_off.p, (nq + 1) * 8, hipMemcpyDeviceToHost, nullptr));
    SA_HIP(host_sync(nullptr));
    if (rc == SA_OK && own.end.p) {
        SA_TRY(copy_d2h(end_out, own.end.as<uint32_t>(), info[0], sa_width, nullptr));
        if (own.start.p) SA_TRY(copy_d2h(start_out, own.start.as<uint32_t>(), info[0], sa_width, nullptr));
        if (own.dist.p) {
            SA_HIP(hipMemcpyAsync(dist_out, own.dist.p, info[0], hipMemcpyDeviceToHost, nullptr));
            SA_HIP(host_sync(nullptr));
        }
    }
    return rc;
}

}  // namespace sa

extern "C" {

int sa_edit_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                   uint64_t pat_bytes, const uint64_t* d_pat_off, uint64_t nq, uint64_t k, uint64_t max_candidates,
                   uint32_t flags, uint64_t* d_off, uint32_t* d_end, uint32_t* d_start, uint8_t* d_dist, uint64_t out_cap,
                   uint64_t info[SA_EDIT_INFO], void* stream) {
    return sa::edit_device(ctx, d_text, n, d_sa, d_pat, pat_bytes, d_pat_off, nq, k, max_candidates, flags, d_off, d_end,
                           d_start, d_dist, out_cap, info, (hipStream_t)stream);
}

int sa_edit(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat, const uint64_t* pat_off,
            uint64_t nq, uint64_t k, uint64_t max_candidates, uint32_t flags, uint64_t* off_out, void* end_out,
            void* start_out, uint8_t* dist_out, uint64_t out_cap, uint64_t info[SA_EDIT_INFO]) {
    return sa::edit_host(text, n, sa, sa_width, pat, pat_off, nq, k, max_candidates, flags, off_out, end_out, start_out,
                         dist_out, out_cap, info);
}

}  // extern "C"

#endif   // __HIPCC__
