// sa_ibwt.h -- the LF-mapping of a BWT and the inverse transform: the text, and
// if asked the suffix array, from (bwt, primary) alone (sa_lf / sa_lf_device,
// sa_ibwt / sa_ibwt_device of include/sa_hip.h).
//
// The convention is sa_bwt.h's: n bytes, no sentinel, bwt[p] = text[n - 1] at
// the primary index p.  LF is the stable one-byte counting sort of the rows in
// the order p, 0, 1, .. p - 1, p + 1, .. n - 1.  With E[c] = the rows other
// than p whose byte is below c and last = bwt[p]:
//   LF[p] = E[last],  LF[r] = E[c] + [last <= c] + #{k < r, k != p, bwt[k] == c}.
// It is a permutation of [0, n) for any bytes and any p < n, so nothing that
// follows it can leave the buffers or run for ever.  first[c] = E[c] +
// [last < c] (first[256] = n) is where byte c starts in the sorted column: the
// byte of a rank is a search over those 257 values, and the walks below need
// LF alone, one 4-byte gather a step.
//
// LF (sa_lf_device: no host wait, asynchronous on the stream):
//   k_lf_hist   one workgroup of kLfBlock = 1024 lanes per tile of kLfTile =
//               32768 ranks; each of its 16 wavefronts counts its own 2048
//               ranks in its own 256 LDS counters (256 ranks a step: one dword
//               per lane, handed round by shuffles so that a step's four
//               rounds are in rank order; the lanes of equal byte found by
//               eight ballots, their lowest lane adds the count: no atomics,
//               and DNA's four hot bytes cost what 256 cost).  Row p counts
//               nowhere.  Out: cnt[c][tile], uint32.
//   k_lf_scan   one workgroup per byte: the exclusive sums of its row of cnt
//               across the tiles, in place, and the byte's total.
//   k_lf_rank   the tile again: the wavefront counts, E from the 256 totals,
//               then every wavefront's counters start at E[c] + [last <= c] +
//               the tiles before + the wavefronts before, and the same
//               match-any step hands out stable ranks: coalesced 256-byte LF
//               stores.  The workgroup that owns p writes LF[p]; workgroup 0
//               writes first[] when asked.
//   The count table is 256 x ceil(n / 32768) uint32: n / 32 bytes, 128 MiB at
//   n = 2^32 (a tile of 4096 would need 1 GiB there).  Traffic: the BWT three
//   times (twice from L2 in k_lf_rank), 4 n bytes out, the table twice.  The
//   BWT may start at any byte (dword loads when it is 4-byte aligned and the
//   dword is whole, byte loads otherwise); d_lf is uint32, so 4-byte aligned.
//
// Inverse (sa_ibwt_device): the chain r_0 = LF[p], r_k = LF[r_{k-1}] spells
// the text backwards, text[n - 1 - k] = the byte of r_k and SA[r_k] = n - 1 -
// k, and (bwt, p) is a BWT exactly when the cycle of r_0 has all n ranks.
// Ranking that cycle is Helman-JaJa list ranking:
//   splitters   r_0 and every rank whose hash r * 0x9E3779B1 mod 2^32 has its
//               top kIbwtSplitBits = 6 bits zero (S = 64), NOT r % S: on the
//               Thue-Morse word the chain meets regular splitters in stretches
//               of 61,727 steps at n = 2^18 and hashed ones in 476 (DESIGN.md
//               section 17).  The hash does not see the data, so no text
//               picks its own bad splitters.
//   k_ibwt_dir  one bit per rank in 64-bit words, the splitters before each
//               word inside its tile of kIbwtTile = 16384 ranks (256 words),
//               the tile's count; scan_i64 over the tile counts.  Compact
//               index of a splitter = tile sum + word count + popcount.
//   k_ibwt_walk1  one lane per splitter (a workgroup takes the splitters of
//               one tile: lane i finds the i-th by a search over the word
//               counts in LDS): follow LF to the next splitter, store
//               (successor's compact index, steps) as one 64-bit node; the
//               sublist that ends at r_0 gets no successor, which cuts the
//               cycle into a list.  One walk per lane: a lane holds one gather
//               in flight and the occupancy (8 wavefronts per SIMD, no LDS to
//               speak of) supplies the rest; two walks per lane were not
//               tried.  The longest sublist goes to an atomic max.
//   k_ibwt_jump Wyllie pointer jumping over the nodes, ceil(log2(cap)) rounds
//               between two buffers (8 bytes per node each, one 8-byte gather
//               per node and round; n / 64 nodes: 128 MiB at 2^30).  Afterwards
//               a node holds the steps from its splitter round to r_0 again:
//               SA[splitter] + 1 for a genuine BWT, and the node of r_0 holds
//               the length of its cycle.
//   k_ibwt_verdict  that length L: valid iff L == n.  Info words for the host.
//   k_ibwt_walk2  the splitters again, each from its text position downwards:
//               the byte of each rank by a search over first[] in LDS, four
//               descending bytes packed into one dword store where the address
//               allows (byte stores at a sublist's ragged ends), so exactly
//               d_text[0, n) is written at any alignment; SA[r] = pos as
//               scattered dword stores when d_sa is given.  It is launched
//               before the host knows the verdict, reads L on the device and
//               writes nothing unless L == n (as k_rep_emit does with out_cap).
//   The number of splitters is known on the device only: the node buffers
//   hold cap = n / 64 + n / 1024 + 1024 (the hash is a Kronecker sequence, its
//   counts stray from n / 64 by a few dozen); every node store is guarded and
//   a count above cap is SA_E_INTERNAL.
//
// Host waits per call.  sa_lf_device: none.  sa_ibwt_device: one (the info
// words, after everything is enqueued).  Temporaries, stream-ordered:
// sa_lf_device n / 32 bytes; sa_ibwt_device about 4.48 n bytes (LF 4 n, the
// count table n / 32, splitter words n / 8, word counts n / 16, two node
// buffers 2 x 8 x cap = 0.27 n, 8 bytes per tile).
//
// Everything up to the HIP part compiles on the host: the LF rule, the
// splitter predicate and directory, both walks with the byte packing, the
// jump and the verdict.  tests/cpp/ibwt_check.cpp runs them against brute
// force.  Measurements and the resource report: DESIGN.md section 17.  The HIP
// part needs sa_host.h, sa_locate.h (LocBuf), sa_query.h (mem_block_excl) and
// sa_build.hip's scan_i64 before it.
#pragma once
#include <stdint.h>

#include "sa_search.h"   // SA_HD

namespace sa {

constexpr uint32_t kLfTile = 32768;            // ranks per row of the count table (= _native.LF_TILE)
constexpr int kIbwtInfo = 3;                   // = SA_IBWT_INFO
constexpr uint32_t kIbwtSplitBits = 6;         // S = 64 (= _native.IBWT_S): one rank in 64 is a splitter
constexpr uint32_t kIbwtHash = 0x9E3779B1u;    // 2^32 / golden ratio, odd
constexpr uint32_t kIbwtNil = 0xFFFFFFFFu;     // no successor
constexpr uint32_t kIbwtWordRanks = 64;        // ranks per word of splitter bits
constexpr uint32_t kIbwtTileWords = 256;       // words per directory tile
constexpr uint32_t kIbwtTile = kIbwtWordRanks * kIbwtTileWords;

// ---- LF ---------------------------------------------------------------------
// e_c = E[c].  Where byte c starts in the sorted column, and where the rows
// other than the primary start in it (the primary row comes first in its byte).
SA_HD uint32_t lf_first(uint32_t e_c, uint32_t c, uint32_t last) { return e_c + (last < c ? 1u : 0u); }
SA_HD uint32_t lf_base(uint32_t e_c, uint32_t c, uint32_t last) { return e_c + (last <= c ? 1u : 0u); }

// the byte whose stretch of the sorted column holds rank q < n: the largest c
// with first[c] <= q (first has 257 entries, first[0] = 0, first[256] = n)
SA_HD uint32_t ibwt_byte_of(const uint32_t* first, uint32_t q) {
    uint32_t lo = 0, hi = 255;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (first[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- splitters --------------------------------------------------------------
// bits in [1, 31]: one rank in 2^bits
SA_HD bool ibwt_hashed(uint32_t r, uint32_t bits) { return ((uint32_t)(r * kIbwtHash) >> (32u - bits)) == 0u; }
SA_HD bool ibwt_is_splitter(uint32_t r, uint32_t r0, uint32_t bits) { return r == r0 || ibwt_hashed(r, bits); }

// word w of the splitter bits: bit k = rank 64 w + k < n is a splitter
SA_HD uint64_t ibwt_split_word(uint64_t w, uint64_t n, uint32_t r0, uint32_t bits) {
    uint64_t m = 0;
    const uint64_t base = w * kIbwtWordRanks;
    for (uint32_t k = 0; k < kIbwtWordRanks; ++k)
        if (base + k < n && ibwt_is_splitter((uint32_t)(base + k), r0, bits)) m |= 1ull << k;
    return m;
}

// Splitters below rank r = the compact index of r when it is one.  d.word(w);
// d.count(w): the splitters of w's tile in front of word w; d.tile(t): those
// of the tiles in front of tile t.  WPT: words per tile.
template <uint32_t WPT, class D>
SA_HD uint32_t ibwt_dir_index(const D& d, uint32_t r) {
    const uint32_t w = r / kIbwtWordRanks;
    const uint64_t m = d.word(w) & ((1ull << (r % kIbwtWordRanks)) - 1ull);
    return (uint32_t)(d.tile(w / WPT) + d.count(w) + (uint64_t)__builtin_popcountll(m));
}

// the rank of the k-th set bit (k < popcount) of word w
SA_HD uint32_t ibwt_select(uint64_t word, uint32_t k, uint32_t w) {
    for (uint32_t q = 0; q < k; ++q) word &= word - 1ull;
    return w * kIbwtWordRanks + (uint32_t)__builtin_ctzll(word);
}

// ---- the list ---------------------------------------------------------------
// a node: the successor's compact index above, a number of steps below
SA_HD uint64_t ibwt_node(uint32_t succ, uint32_t d) { return ((uint64_t)succ << 32) | d; }
SA_HD uint32_t ibwt_succ(uint64_t x) { return (uint32_t)(x >> 32); }
SA_HD uint32_t ibwt_dist(uint64_t x) { return (uint32_t)x; }

// Walk 1 from splitter s: the steps to the next splitter (>= 1; at most n, LF
// being a permutation), which is `end`.  lf(r) = LF[r].
template <class LF>
SA_HD uint32_t ibwt_walk1(const LF& lf, uint32_t s, uint32_t r0, uint32_t bits, uint64_t n, uint32_t& end) {
    uint32_t r = s;
    uint64_t steps = 0;
    do {
        r = lf(r);
        ++steps;
    } while (!ibwt_is_splitter(r, r0, bits) && steps < n);
    end = r;
    return (uint32_t)steps;
}

// one round of pointer jumping: node x of the previous round's array `in`
SA_HD uint64_t ibwt_jump(const uint64_t* in, uint64_t x) {
    const uint32_t succ = ibwt_succ(x);
    if (succ == kIbwtNil) return x;
    const uint64_t y = in[succ];
    return ibwt_node(ibwt_succ(y), ibwt_dist(x) + ibwt_dist(y));   // wraps on the cycles of an invalid input only
}

// rounds after which a list of at most m nodes has no successor left: 2^R >= m
SA_HD int ibwt_rounds(uint64_t m) {
    int r = 0;
    while ((1ull << r) < m) ++r;
    return r;
}

// node buffers are allocated for this many splitters
SA_HD uint64_t ibwt_node_cap(uint64_t n) { return (n >> kIbwtSplitBits) + (n >> 10) + 1024; }

// Walk 2 from splitter s at text position pos = SA[s]: the bytes of s, LF[s],
// .. up to the next splitter go to positions pos, pos - 1, ..; `addr` is the
// address of text[0] (its low two bits decide what a dword is).  o.word(q, x):
// the four bytes of x to positions q .. q + 3, lowest first (address of q is
// 4-byte aligned); o.byte(q, b); o.sa(r, q).
template <class LF, class Out>
SA_HD void ibwt_walk2(const LF& lf, const uint32_t* first, uint32_t s, uint32_t pos, uint32_t r0, uint32_t bits,
                      uint64_t n, uint64_t addr, Out& o) {
    uint32_t r = s, acc = 0, have = 0;
    uint64_t steps = 0;
    for (;;) {
        acc = (acc << 8) | ibwt_byte_of(first, r);   // the byte of position pos + k is bits 8 k .. of acc
        ++have;
        o.sa(r, pos);
        if (((addr + pos) & 3u) == 0u) {
            if (have == 4) o.word(pos, acc);
            else
                for (uint32_t k = 0; k < have; ++k) o.byte(pos + k, (acc >> (8 * k)) & 255u);
            have = 0;
        }
        r = lf(r);
        ++steps;
        if (ibwt_is_splitter(r, r0, bits) || steps >= n || pos == 0) break;
        --pos;
    }
    for (uint32_t k = 0; k < have; ++k) o.byte(pos + k, (acc >> (8 * k)) & 255u);
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

#include "sa_kernels.h"

namespace sa {

static_assert(SA_IBWT_INFO == kIbwtInfo, "sa_hip.h states it");
constexpr int kLfBlock = 1024;                                  // lanes of an LF workgroup
constexpr int kLfWaves = kLfBlock / kWave;                      // 16
constexpr uint32_t kLfWaveRanks = kLfTile / kLfWaves;           // 2048 ranks per wavefront
constexpr uint32_t kLfStep = 4 * kWave;                         // 256 ranks a step: one dword per lane
constexpr int kIbwtDevInfo = 4;                                 // device info words: splitters, longest, L, unused
static_assert(kLfWaveRanks % kLfStep == 0 && kIbwtTileWords == (uint32_t)kBlock, "whole steps; a lane per word");

// four BWT bytes from rank r (a multiple of 4), zero past n
__device__ __forceinline__ uint32_t lf_load4(const uint8_t* __restrict__ bwt, uint64_t r, uint64_t n, bool aligned) {
    if (aligned && r + 4 <= n) return *reinterpret_cast<const uint32_t*>(bwt + r);
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (r + k < n) w |= (uint32_t)bwt[r + k] << (8 * k);
    return w;
}

// the valid lanes of this wavefront whose c equals this lane's (for a valid lane)
__device__ __forceinline__ uint64_t lf_match(uint32_t c, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (c >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// One wavefront over its kLfWaveRanks ranks from `sub`, in rank order: s_c[c]
// += the rows of byte c; RANK: lf[r] = s_c[c] as it stood when row r came.
// Only this wavefront touches s_c, and a step's leaders have distinct bytes.
template <bool RANK>
__device__ __forceinline__ void lf_wave_pass(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t p, bool aligned,
                                             uint64_t sub, uint32_t* s_c, uint32_t* __restrict__ lf) {
    const uint32_t lane = lane_id();
    for (uint32_t step = 0; step < kLfWaveRanks / kLfStep; ++step) {
        const uint64_t b0 = sub + (uint64_t)step * kLfStep;
        if (b0 >= n) break;   // uniform
        const uint32_t word = lf_load4(bwt, b0 + 4u * lane, n, aligned);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t w = (uint32_t)__shfl((int)word, (int)(16u * j + (lane >> 2)), kWave);
            const uint32_t c = (w >> (8u * (lane & 3u))) & 255u;
            const uint64_t r = b0 + 64u * j + lane;
            const bool valid = r < n && r != p;
            const uint64_t m = lf_match(c, valid);
            const uint32_t lead = valid ? (uint32_t)__builtin_ctzll(m) : lane;
            uint32_t old = 0;
            if (valid && lead == lane) {
                old = s_c[c];
                s_c[c] = old + (uint32_t)__popcll(m);
            }
            if (RANK) {
                old = (uint32_t)__shfl((int)old, (int)lead, kWave);
                if (valid) lf[r] = old + (uint32_t)__popcll(m & lanemask_lt());
            }
        }
    }
}

// cnt[c * tiles + tile] = the rows of byte c in the tile, row p apart
__global__ __launch_bounds__(kLfBlock) void k_lf_hist(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t p,
                                                      uint32_t aligned, uint32_t* __restrict__ cnt, uint32_t tiles) {
    __shared__ uint32_t s_c[kLfWaves * 256];
    const uint32_t tid = threadIdx.x, wave = tid / kWave;
    for (uint32_t i = tid; i < kLfWaves * 256; i += kLfBlock) s_c[i] = 0u;
    __syncthreads();
    lf_wave_pass<false>(bwt, n, p, aligned != 0, (uint64_t)blockIdx.x * kLfTile + wave * kLfWaveRanks, s_c + wave * 256,
                        nullptr);
    __syncthreads();
    if (tid < 256) {
        uint32_t x = 0;
#pragma unroll
        for (int w = 0; w < kLfWaves; ++w) x += s_c[w * 256 + tid];
        cnt[(uint64_t)tid * tiles + blockIdx.x] = x;
    }
}

// row c of cnt becomes its exclusive sums; totals[c] = its sum
__global__ __launch_bounds__(kBlock) void k_lf_scan(uint32_t* __restrict__ cnt, uint32_t tiles,
                                                    uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_w[kWaves];
    uint32_t* row = cnt + (uint64_t)blockIdx.x * tiles;
    const uint32_t per = (tiles + kBlock - 1) / kBlock;
    const uint32_t a = std::min<uint32_t>(threadIdx.x * per, tiles), e = std::min<uint32_t>(a + per, tiles);
    uint32_t x = 0;
    for (uint32_t i = a; i < e; ++i) x += row[i];
    uint32_t sum;
    uint32_t run = mem_block_excl(x, s_w, sum);
    for (uint32_t i = a; i < e; ++i) {
        const uint32_t y = row[i];
        row[i] = run;
        run += y;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = sum;
}

// first: 257 words or NULL
__global__ __launch_bounds__(kLfBlock) void k_lf_rank(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t p,
                                                      uint32_t aligned, const uint32_t* __restrict__ cnt, uint32_t tiles,
                                                      const uint32_t* __restrict__ totals, uint32_t* __restrict__ lf,
                                                      uint32_t* __restrict__ first) {
    __shared__ uint32_t s_c[kLfWaves * 256];
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, wave = tid / kWave, lane = lane_id();
    const uint64_t sub = (uint64_t)blockIdx.x * kLfTile + wave * kLfWaveRanks;
    const uint32_t last = bwt[p];
    for (uint32_t i = tid; i < kLfWaves * 256; i += kLfBlock) s_c[i] = 0u;
    __syncthreads();
    lf_wave_pass<false>(bwt, n, p, aligned != 0, sub, s_c + wave * 256, nullptr);
    // E[tid] for tid < 256: the exclusive sums of the totals (wavefronts 0 .. 3)
    const uint32_t v = tid < 256 ? totals[tid] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o, kWave);
        if ((int)lane >= o) incl += y;
    }
    if (wave < 4 && lane == kWave - 1) s_w[wave] = incl;
    __syncthreads();   // s_w, and every wavefront's counts
    if (tid < 256) {
        uint32_t e = incl - v;
        for (uint32_t q = 0; q < wave; ++q) e += s_w[q];
        if (blockIdx.x == 0 && first) {
            first[tid] = lf_first(e, tid, last);
            if (tid == 255) first[256] = (uint32_t)n;
        }
        if (tid == last && p / kLfTile == blockIdx.x) lf[p] = e;
        uint32_t run = lf_base(e, tid, last) + cnt[(uint64_t)tid * tiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < kLfWaves; ++w) {
            const uint32_t t = s_c[w * 256 + tid];
            s_c[w * 256 + tid] = run;
            run += t;
        }
    }
    __syncthreads();
    lf_wave_pass<true>(bwt, n, p, aligned != 0, sub, s_c + wave * 256, lf);
}

// the splitter directory in device memory: tinc = the inclusive sums of the tiles' counts
struct IbwtDir {
    const uint64_t* __restrict__ words;
    const uint32_t* __restrict__ wcnt;
    const int64_t* __restrict__ tinc;
    __device__ __forceinline__ uint64_t word(uint32_t w) const { return words[w]; }
    __device__ __forceinline__ uint64_t count(uint32_t w) const { return wcnt[w]; }
    __device__ __forceinline__ uint64_t tile(uint32_t t) const { return t ? (uint64_t)tinc[t - 1] : 0; }
};

struct IbwtLf {
    const uint32_t* __restrict__ lf;
    __device__ __forceinline__ uint32_t operator()(uint32_t r) const { return lf[r]; }
};

// one workgroup per tile of kIbwtTile ranks, a lane per word (the arrays hold whole tiles)
__global__ __launch_bounds__(kBlock) void k_ibwt_dir(const uint32_t* __restrict__ lf, uint32_t p, uint64_t n,
                                                     uint64_t* __restrict__ words, uint32_t* __restrict__ wcnt,
                                                     int64_t* __restrict__ tcnt) {
    __shared__ uint32_t s_w[kWaves];
    const uint32_t r0 = lf[p];
    const uint64_t w = (uint64_t)blockIdx.x * kIbwtTileWords + threadIdx.x;
    const uint64_t m = ibwt_split_word(w, n, r0, kIbwtSplitBits);
    uint32_t sum;
    const uint32_t before = mem_block_excl((uint32_t)__popcll(m), s_w, sum);
    words[w] = m;
    wcnt[w] = before;
    if (threadIdx.x == 0) tcnt[blockIdx.x] = (int64_t)sum;
}

// The splitters of tile t into LDS form: s_word / s_pre get the tile's words
// and word counts; returns how many there are.  Ends with a barrier.
__device__ __forceinline__ uint32_t ibwt_tile_load(const IbwtDir& d, uint32_t t, uint64_t* s_word, uint32_t* s_pre) {
    const uint32_t w = t * kIbwtTileWords + threadIdx.x;
    s_word[threadIdx.x] = d.words[w];
    s_pre[threadIdx.x] = d.wcnt[w];
    __syncthreads();
    return (uint32_t)((uint64_t)d.tinc[t] - d.tile(t));
}

// the i-th splitter of the tile (i < its count)
__device__ __forceinline__ uint32_t ibwt_tile_pick(const uint64_t* s_word, const uint32_t* s_pre, uint32_t t, uint32_t i) {
    uint32_t lo = 0, hi = kIbwtTileWords - 1;   // the largest word with s_pre <= i: it holds splitter i
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (s_pre[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return ibwt_select(s_word[lo], i - s_pre[lo], t * kIbwtTileWords + lo);
}

// dinfo[1] = the longest sublist (zeroed before)
__global__ __launch_bounds__(kBlock) void k_ibwt_walk1(IbwtLf lf, uint32_t p, uint64_t n, IbwtDir d,
                                                       uint64_t* __restrict__ nodes, uint64_t cap,
                                                       unsigned long long* __restrict__ dinfo) {
    __shared__ uint64_t s_word[kIbwtTileWords];
    __shared__ uint32_t s_pre[kIbwtTileWords];
    const uint32_t t = blockIdx.x;
    const uint32_t r0 = lf(p);
    const uint32_t count = ibwt_tile_load(d, t, s_word, s_pre);
    const uint64_t j0 = d.tile(t);
    uint32_t longest = 0;
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
        const uint32_t s = ibwt_tile_pick(s_word, s_pre, t, i);
        uint32_t end;
        const uint32_t len = ibwt_walk1(lf, s, r0, kIbwtSplitBits, n, end);
        const uint32_t succ = end == r0 ? kIbwtNil : ibwt_dir_index<kIbwtTileWords>(d, end);
        if (j0 + i < cap) nodes[j0 + i] = ibwt_node(succ, len);
        longest = std::max(longest, len);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) longest = std::max(longest, (uint32_t)__shfl_xor((int)longest, o, kWave));
    if (lane_id() == 0 && longest) atomicMax(&dinfo[1], (unsigned long long)longest);
}

// m: the number of splitters, on the device
__global__ __launch_bounds__(kBlock) void k_ibwt_jump(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                      const int64_t* __restrict__ m, uint64_t cap) {
    const uint64_t count = (uint64_t)*m;
    if (count > cap) return;
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < count) out[j] = ibwt_jump(in, in[j]);
}

// dinfo: [0] splitters, [2] the length of r_0's cycle (0 when the nodes did not fit)
__global__ void k_ibwt_verdict(IbwtLf lf, uint32_t p, IbwtDir d, const uint64_t* __restrict__ nodes,
                               const int64_t* __restrict__ m, uint64_t cap, unsigned long long* __restrict__ dinfo) {
    if (threadIdx.x) return;
    const uint64_t count = (uint64_t)*m;
    dinfo[0] = count;
    dinfo[2] = count > cap ? 0ull : (unsigned long long)ibwt_dist(nodes[ibwt_dir_index<kIbwtTileWords>(d, lf(p))]);
}

struct IbwtOut {
    uint8_t* __restrict__ text;
    uint32_t* __restrict__ sa_out;   // or NULL
    __device__ __forceinline__ void word(uint32_t q, uint32_t x) const { *reinterpret_cast<uint32_t*>(text + q) = x; }
    __device__ __forceinline__ void byte(uint32_t q, uint32_t b) const { text[q] = (uint8_t)b; }
    __device__ __forceinline__ void sa(uint32_t r, uint32_t q) const {
        if (sa_out) sa_out[r] = q;
    }
};

// nodes: after the last round.  Silent unless dinfo[2] == n.
__global__ __launch_bounds__(kBlock) void k_ibwt_walk2(IbwtLf lf, uint32_t p, uint64_t n, IbwtDir d,
                                                       const uint64_t* __restrict__ nodes,
                                                       const uint32_t* __restrict__ first,
                                                       const unsigned long long* __restrict__ dinfo, IbwtOut o) {
    __shared__ uint64_t s_word[kIbwtTileWords];
    __shared__ uint32_t s_pre[kIbwtTileWords];
    __shared__ uint32_t s_first[257];
    if (dinfo[2] != n) return;   // uniform: not a BWT, nothing is written
    const uint32_t t = blockIdx.x;
    const uint32_t r0 = lf(p);
    for (uint32_t i = threadIdx.x; i < 257; i += kBlock) s_first[i] = first[i];
    const uint32_t count = ibwt_tile_load(d, t, s_word, s_pre);
    const uint64_t j0 = d.tile(t);
    const uint64_t addr = (uint64_t)(uintptr_t)o.text;
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
        const uint32_t s = ibwt_tile_pick(s_word, s_pre, t, i);
        const uint32_t dist = ibwt_dist(nodes[j0 + i]);   // steps from s round to r_0 = SA[s] + 1
        if (dist == 0 || dist > n) continue;              // (cannot be when the cycle has n ranks)
        ibwt_walk2(lf, s_first, s, dist - 1u, r0, kIbwtSplitBits, n, addr, o);
    }
}

// LF of (d_bwt, p) into d_lf, first[] (257 words) into d_first when given; n >= 1, p < n
static int lf_launch(const uint8_t* d_bwt, uint64_t n, uint64_t p, uint32_t* d_lf, uint32_t* d_first, hipStream_t s) {
    const uint32_t tiles = (uint32_t)((n + kLfTile - 1) / kLfTile);   // <= 2^17
    LocBuf tmp;
    SA_TRY(tmp.alloc(((uint64_t)tiles * 256 + 256) * 4, s));
    uint32_t* d_cnt = (uint32_t*)tmp.p;
    uint32_t* d_tot = d_cnt + (uint64_t)tiles * 256;
    const uint32_t aligned = ((uintptr_t)d_bwt & 3u) == 0u;
    hipLaunchKernelGGL(k_lf_hist, dim3(tiles), dim3(kLfBlock), 0, s, d_bwt, n, p, aligned, d_cnt, tiles);
    hipLaunchKernelGGL(k_lf_scan, dim3(256), dim3(kBlock), 0, s, d_cnt, tiles, d_tot);
    hipLaunchKernelGGL(k_lf_rank, dim3(tiles), dim3(kLfBlock), 0, s, d_bwt, n, p, aligned, (const uint32_t*)d_cnt, tiles,
                       (const uint32_t*)d_tot, d_lf, d_first);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// the checks of sa_lf_device, all before any HIP call
static int lf_check_args(const sa_context* c, const uint8_t* d_bwt, uint64_t n, uint64_t primary, const uint32_t* d_lf) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (n == 0) return SA_OK;
    if (!d_bwt) return set_err(SA_E_INVALID, "d_bwt is NULL");
    if (!d_lf) return set_err(SA_E_INVALID, "d_lf is NULL");
    if (primary >= n) return set_err(SA_E_INVALID, "primary index %llu is not below n", (unsigned long long)primary);
    if ((const void*)d_lf == (const void*)d_bwt) return set_err(SA_E_INVALID, "d_lf may not alias d_bwt");
    if ((uintptr_t)d_lf & 3u) return set_err(SA_E_INVALID, "d_lf is not 4-byte aligned");
    return SA_OK;
}

// Host waits: none.
static int lf_device(sa_context* c, const uint8_t* d_bwt, uint64_t n, uint64_t primary, uint32_t* d_lf, hipStream_t s) {
    SA_TRY(lf_check_args(c, d_bwt, n, primary, d_lf));
    if (n == 0) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    return lf_launch(d_bwt, n, primary, d_lf, nullptr, s);
}

// the checks of sa_ibwt_device, all before any HIP call
static int ibwt_check_args(const sa_context* c, const uint8_t* d_bwt, uint64_t n, uint64_t primary, const uint8_t* d_text,
                           const uint32_t* d_sa) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (n == 0) return SA_OK;
    if (!d_bwt) return set_err(SA_E_INVALID, "d_bwt is NULL");
    if (!d_text) return set_err(SA_E_INVALID, "d_text is NULL");
    if (primary >= n) return set_err(SA_E_INVALID, "primary index %llu is not below n", (unsigned long long)primary);
    if (d_text == d_bwt) return set_err(SA_E_INVALID, "d_text may not alias d_bwt");
    SA_TRY(check_no_alias({d_sa}, {d_bwt, d_text}, "d_sa may not alias d_bwt or d_text"));
    if ((uintptr_t)d_sa & 3u) return set_err(SA_E_INVALID, "d_sa is not 4-byte aligned");
    return SA_OK;
}

// Host waits: one, for the info words.
static int ibwt_device(sa_context* c, const uint8_t* d_bwt, uint64_t n, uint64_t primary, uint8_t* d_text, uint32_t* d_sa,
                       uint64_t* info, hipStream_t s) {
    SA_TRY(ibwt_check_args(c, d_bwt, n, primary, d_text, d_sa));
    if (info) info[0] = info[1] = info[2] = 0;
    if (n == 0) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    const uint32_t p = (uint32_t)primary;
    const uint32_t tiles = (uint32_t)((n + kIbwtTile - 1) / kIbwtTile);   // <= 2^18
    const uint64_t words = (uint64_t)tiles * kIbwtTileWords;
    const uint64_t cap = ibwt_node_cap(n);
    // nodes (8, two buffers) | splitter words (8) | tile counts (8) | device info (8) | LF (4) | word counts (4) | first (4)
    const uint64_t b_nodes = cap * 8, b_words = words * 8, b_tile = (uint64_t)tiles * 8, b_info = kIbwtDevInfo * 8,
                   b_lf = align_up(n, 64) * 4, b_wcnt = words * 4, b_first = 260 * 4;
    LocBuf tmp;
    SA_TRY(tmp.alloc(2 * b_nodes + b_words + b_tile + b_info + b_lf + b_wcnt + b_first, s));
    uint64_t* d_na = (uint64_t*)tmp.p;
    uint64_t* d_nb = d_na + cap;
    uint64_t* d_words = d_nb + cap;
    int64_t* d_tcnt = (int64_t*)(d_words + words);
    unsigned long long* d_info = (unsigned long long*)(d_tcnt + tiles);
    uint32_t* d_lf = (uint32_t*)(d_info + kIbwtDevInfo);
    uint32_t* d_wcnt = (uint32_t*)((uint8_t*)d_lf + b_lf);
    uint32_t* d_first = d_wcnt + words;
    SA_TRY(lf_launch(d_bwt, n, p, d_lf, d_first, s));
    SA_HIP(hipMemsetAsync(d_info, 0, b_info, s));
    hipLaunchKernelGGL(k_ibwt_dir, dim3(tiles), dim3(kBlock), 0, s, (const uint32_t*)d_lf, p, n, d_words, d_wcnt, d_tcnt);
    SA_HIP(hipGetLastError());
    SA_TRY(scan_i64<ScanSum>(d_tcnt, tiles, s));
    const IbwtLf lf{d_lf};
    const IbwtDir dir{d_words, d_wcnt, d_tcnt};
    const int64_t* d_m = d_tcnt + (tiles - 1);
    hipLaunchKernelGGL(k_ibwt_walk1, dim3(tiles), dim3(kBlock), 0, s, lf, p, n, dir, d_na, cap, d_info);
    const int rounds = ibwt_rounds(cap);
    for (int k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(k_ibwt_jump, dim3((uint32_t)((cap + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           (const uint64_t*)d_na, d_nb, d_m, cap);
        std::swap(d_na, d_nb);
    }
    hipLaunchKernelGGL(k_ibwt_verdict, dim3(1), dim3(kWave), 0, s, lf, p, dir, (const uint64_t*)d_na, d_m, cap, d_info);
    hipLaunchKernelGGL(k_ibwt_walk2, dim3(tiles), dim3(kBlock), 0, s, lf, p, n, dir, (const uint64_t*)d_na,
                       (const uint32_t*)d_first, (const unsigned long long*)d_info, IbwtOut{d_text, d_sa});
    SA_HIP(hipGetLastError());
    uint64_t* h = host_u64<kHwIbwt, kIbwtDevInfo>(c);
    SA_HIP(hipMemcpyAsync(h, d_info, b_info, hipMemcpyDeviceToHost, s));
    SA_HIP(host_sync(s));
    SA_TRACE("ibwt: %llu splitters (cap %llu), longest sublist %llu, cycle of r0 %llu of %llu", (unsigned long long)h[0],
             (unsigned long long)cap, (unsigned long long)h[1], (unsigned long long)h[2], (unsigned long long)n);
    if (h[0] > cap) return set_err(SA_E_INTERNAL, "%llu splitters do not fit %llu nodes", (unsigned long long)h[0],
                                   (unsigned long long)cap);
    if (info) {
        info[0] = h[0];
        info[1] = h[1];
        info[2] = h[2] - 1;   // the primary row is the last rank of the cycle of r_0
    }
    if (h[2] != n)
        return set_err(SA_E_INVALID, "not a BWT: the chain from LF[primary] closes after %llu of %llu ranks",
                       (unsigned long long)h[2], (unsigned long long)n);
    return SA_OK;
}

// host in, host out (sa_lf), over the steps of sa_host.h
static int lf_host(const uint8_t* bwt, uint64_t n, uint64_t primary, void* lf_out, int width) {
    SA_TRY(check_width(width));
    SA_TRY(check_n32(n));
    if (n == 0) return SA_OK;
    if (!bwt || !lf_out) return set_err(SA_E_INVALID, "NULL host pointer");
    if (primary >= n) return set_err(SA_E_INVALID, "primary index %llu is not below n", (unsigned long long)primary);
    if ((const void*)bwt == (const void*)lf_out) return set_err(SA_E_INVALID, "lf_out may not alias bwt");
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_bwt, d_lf;
    SA_TRY(d_bwt.alloc(align_up(n, 256)));
    SA_TRY(d_lf.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{d_bwt.p, bwt, n}}));
    SA_TRY(lf_device(c, d_bwt.as<uint8_t>(), n, primary, d_lf.as<uint32_t>(), nullptr));
    return copy_d2h(lf_out, d_lf.as<uint32_t>(), n, width, nullptr);
}

// host in, host out (sa_ibwt)
static int ibwt_host(const uint8_t* bwt, uint64_t n, uint64_t primary, uint8_t* text_out, void* sa_out, int sa_width,
                     uint64_t* info) {
    if (info) info[0] = info[1] = info[2] = 0;
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (n == 0) return SA_OK;
    if (!bwt || !text_out) return set_err(SA_E_INVALID, "NULL host pointer");
    if (primary >= n) return set_err(SA_E_INVALID, "primary index %llu is not below n", (unsigned long long)primary);
    if (text_out == bwt) return set_err(SA_E_INVALID, "text_out may not alias bwt");
    SA_TRY(check_no_alias({sa_out}, {bwt, text_out}, "sa_out may not alias bwt or text_out"));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_bwt, d_text, d_sa;
    SA_TRY(d_bwt.alloc(align_up(n, 256)));
    SA_TRY(d_text.alloc(align_up(n, 256)));
    if (sa_out) SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{d_bwt.p, bwt, n}}));
    SA_TRY(ibwt_device(c, d_bwt.as<uint8_t>(), n, primary, d_text.as<uint8_t>(), d_sa.as<uint32_t>(), info, nullptr));
    if (hipMemcpyAsync(text_out, d_text.p, n, hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
        host_sync(nullptr) != hipSuccess)
        return set_err(SA_E_HIP, "D2H copy failed: %s", hipGetErrorString(hipGetLastError()));
    if (sa_out) SA_TRY(copy_d2h(sa_out, d_sa.as<uint32_t>(), n, sa_width, nullptr));
    return SA_OK;
}

}  // namespace sa

extern "C" {

int sa_lf_device(sa_context* ctx, const uint8_t* d_bwt, uint64_t n, uint64_t primary, uint32_t* d_lf, void* stream) {
    return sa::lf_device(ctx, d_bwt, n, primary, d_lf, (hipStream_t)stream);
}

int sa_ibwt_device(sa_context* ctx, const uint8_t* d_bwt, uint64_t n, uint64_t primary, uint8_t* d_text, uint32_t* d_sa,
                   uint64_t* info, void* stream) {
    return sa::ibwt_device(ctx, d_bwt, n, primary, d_text, d_sa, info, (hipStream_t)stream);
}

int sa_lf(const uint8_t* bwt, uint64_t n, uint64_t primary, void* lf_out, int width) {
    return sa::lf_host(bwt, n, primary, lf_out, width);
}

int sa_ibwt(const uint8_t* bwt, uint64_t n, uint64_t primary, uint8_t* text_out, void* sa_out, int sa_width) {
    return sa::ibwt_host(bwt, n, primary, text_out, sa_out, sa_width, nullptr);
}

int sa_ibwt_ex(const uint8_t* bwt, uint64_t n, uint64_t primary, uint8_t* text_out, void* sa_out, int sa_width,
               uint64_t* info) {
    return sa::ibwt_host(bwt, n, primary, text_out, sa_out, sa_width, info);
}

}  // extern "C"

#endif   // __HIPCC__
