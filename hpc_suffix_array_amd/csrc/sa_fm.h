// sa_fm.h -- an FM-index over (bwt, primary): backward-search counting and
// locating through a sampled suffix array, with neither the text nor the SA in
// memory (sa_fm_build / sa_fm_count / sa_fm_locate and their _device forms of
// include/sa_hip.h).
//
// The conventions are sa_bwt.h's and sa_ibwt.h's: n bytes, no sentinel, the
// primary index p < n with bwt[p] = text[n - 1] = last.  C[c] = the bytes below
// c in the BWT (C[256] = n), base[c] = C[c] + [c == last] (lf_base), occ(c, r) =
// #{k < r : bwt[k] == c} with row p counted, occ'(c, r) = occ(c, r) - [c == last
// and r > p]: the checkpoints count the plain BWT and row p, which has no suffix
// to its left, is taken out by one comparison.
//   search    P[0, m): lo = C[c], hi = C[c + 1] for c = P[m - 1] (C, not base:
//             the one-byte suffix n - 1 does match a one-byte pattern); then for
//             c = P[m - 2] .. P[0] while lo < hi: x = base[c] + occ'(c, x) for
//             both ends.  hi > lo: exactly sa_find's interval.  Nothing matches:
//             (0, 0), NOT sa_find's insertion point.  m == 0: [0, n).
//   LF        LF[r] = base[bwt[r]] + occ'(bwt[r], r), r != p.
//   locate    row r is marked iff SA[r] % s == 0 (row p always is), sample[rank1
//             (r)] = SA[r] / s; q = r, k = 0; while q is unmarked: q = LF[q], ++k;
//             SA[r] = s * sample[rank1(q)] + k.  At most s - 1 steps, never LF
//             at p.
//
// The index is one position-independent byte buffer (offsets, never pointers;
// every section starts at a multiple of 16 bytes, and so must the buffer):
//   header    kFmHeaderBytes = 4096: FmHeader below (magic, version, n, p, last,
//             sigma, class, s, the sections, col[256] byte -> column or
//             kFmAbsent, C[257], base[256]), zero-padded.
//   blocks    n / R + 1 records of [cols x uint32 occ counts of the rows in
//             front of the block][R raw BWT bytes, zero past n]:
//                 sigma <= 4: cols 4, R 64 (80 bytes);  <= 16: 16, 256 (320);
//                 more: 256, 4096 (5120).
//             The checkpoints cost n / 4 in every class.  The record n / R is
//             there even when it has no row, so occ(c, n) needs no special case.
//   marks     (s > 0) one bit per row in 64-bit words, whole tiles of kIbwtTile
//             rows as in k_ibwt_dir; uint32 marks in front of each word inside
//             its tile; uint64 exclusive sums of the tiles' counts, tiles + 1.
//   samples   (s > 0) ceil(n / s) uint32.
// sa_fm_index_bytes(n, s) is the largest of the three classes' sizes, so that a
// caller allocates before sigma is known: for s = 32 about 1.5625 n + 17 KiB.
//
// Kernels:
//   k_lf_hist / k_lf_scan (sa_ibwt.h)  the byte counts per tile of kLfTile rows,
//               row p apart, their exclusive sums and the totals.  The host
//               waits for the totals and bwt[p]: sigma decides the class.
//   k_fm_header the header, composed on the host, passed by value.
//   k_fm_records one workgroup per tile of kLfTile rows: the rows of each block
//               and column counted in LDS (2048 counters in every class), summed
//               over the tile's blocks, written with the tile's base as the
//               records' counts; the payload copied by dwords.
//   k_fm_marks  a workgroup per tile of kIbwtTile rows, a ballot per word:
//               coalesced SA loads; words, word counts, tile counts (scan_i64).
//   k_fm_samples the same ballots again: sample[tile + word + lanes below] = SA /
//               s, guarded (an SA that is none may mark more than ceil(n / s)).
//   k_fm_count<G>  G = 1 / 4 / 64 lanes per query by class, so that a lane never
//               scans more than 64 payload bytes: up to four 16-byte loads, SWAR
//               byte equality, popcount, a reduction over the G lanes.  Two
//               dependent gathers per pattern byte.  All three are launched and
//               the two of another class return at once: the class is read on
//               the device, there is no host wait.  The kernel checks the header
//               (fm_view) against index_bytes itself: a buffer that is no index
//               answers (0, 0) everywhere; every computed row is clamped to n, a
//               column to cols, a sample index to the samples, so no load leaves
//               d_index[0, index_bytes) whatever the bytes are, and a search ends
//               after m steps, a walk after s.
//   k_fm_loc_count  c[q] as sa_locate.h's, n read from the index; scan_i64.
//   k_fm_resolve<G>  G lanes per hit: the walk above, bounded at s steps, result
//               clamped below n.  In SA order straight into d_pos; otherwise
//               into a buffer of `total` entries that sa_locate.h's machinery
//               sorts per query as an SA of its own with the intervals [off[q],
//               off[q + 1]).
//
// Host waits per call.  sa_fm_build_device: one (the totals; everything after it
// is enqueued and not waited for).  sa_fm_count_device: none.
// sa_fm_locate_device: one for the total and the header's words, then
// sa_locate_device's own over the materialised hits (one when no query is large),
// or one at the end in SA order.  Temporaries, stream-ordered: build n / 32 + 1
// KiB (the count table); count none; locate 4 bytes per hit + 8 nq, and
// sa_locate_device's.
//
// Everything up to the HIP part compiles on the host: the class rule, the size
// arithmetic, the header and its check, record addressing, occ' with the SWAR
// count and the partial-word mask, one backward step, the search, the LF step
// and the locate walk.  tests/cpp/fm_check.cpp runs them against brute force.
// Measurements and the resource report: DESIGN.md section 18.  The HIP part
// needs sa_host.h, sa_find.h (find_pattern), sa_locate.h, sa_query.h (mem_block_excl,
// ListSort) and sa_ibwt.h before it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sa_ibwt.h"     // lf_base, ibwt_dir_index, the directory's shape
#include "sa_locate.h"   // locate_count, locate_lower_bound

namespace sa {

constexpr uint64_t kFmMagic = 0x31584449464D4153ull;   // "SAMFIDX1", little-endian
constexpr uint32_t kFmVersion = 1;
constexpr int kFmInfo = 4;                     // = SA_FM_INFO: sigma, class, bytes used, samples
constexpr uint32_t kFmMaxSample = 4096;        // = SA_FM_MAX_SAMPLE
constexpr uint32_t kFmHeaderBytes = 4096;
constexpr uint32_t kFmAbsent = 0xFFFFu;        // col[c] of a byte the text lacks
constexpr uint32_t kFmPiece = 64;              // payload bytes one lane scans
constexpr uint32_t kFmClasses = 3;

// ---- the class and its record -------------------------------------------------
SA_HD uint32_t fm_class(uint32_t sigma) { return sigma <= 4 ? 0u : sigma <= 16 ? 1u : 2u; }
SA_HD uint32_t fm_cols(uint32_t cls) { return cls == 0 ? 4u : cls == 1 ? 16u : 256u; }
SA_HD uint32_t fm_rows(uint32_t cls) { return cls == 0 ? 64u : cls == 1 ? 256u : 4096u; }   // = _native.FM_ROWS
SA_HD uint32_t fm_lanes(uint32_t cls) { return fm_rows(cls) / kFmPiece; }                   // 1, 4, 64
SA_HD uint32_t fm_record_bytes(uint32_t cls) { return fm_cols(cls) * 4u + fm_rows(cls); }
SA_HD uint64_t fm_align16(uint64_t x) { return (x + 15ull) & ~15ull; }

struct FmHeader {
    uint64_t magic;
    uint32_t version, cls;
    uint64_t n, p;
    uint32_t last, sigma, sample, cols, rows, rec;
    uint64_t bytes;                     // of the whole index
    uint64_t off_blocks, n_blocks;      // records
    uint64_t off_words, n_words;        // mark words
    uint64_t off_wcnt;                  // uint32 per word
    uint64_t off_tiles, n_tiles;        // uint64, n_tiles + 1 entries
    uint64_t off_samples, n_samples;
    uint16_t col[256];
    uint32_t C[257];
    uint32_t base[256];
    uint32_t pad;
};
static_assert(sizeof(FmHeader) <= kFmHeaderBytes && sizeof(FmHeader) % 8 == 0, "the header fits its section");

// the sections of an index of n rows in class cls with sample rate s (0: none)
SA_HD void fm_layout(FmHeader& h, uint64_t n, uint32_t cls, uint32_t s) {
    h.cls = cls;
    h.cols = fm_cols(cls);
    h.rows = fm_rows(cls);
    h.rec = fm_record_bytes(cls);
    h.sample = s;
    uint64_t off = kFmHeaderBytes;
    h.off_blocks = off;
    h.n_blocks = n / h.rows + 1;
    off += h.n_blocks * h.rec;
    h.off_words = h.n_words = h.off_wcnt = h.off_tiles = h.n_tiles = h.off_samples = h.n_samples = 0;
    if (s) {
        h.n_tiles = (n + kIbwtTile - 1) / kIbwtTile;
        h.n_words = h.n_tiles * kIbwtTileWords;
        h.off_words = off;
        off += h.n_words * 8;
        h.off_wcnt = off;
        off = fm_align16(off + h.n_words * 4);
        h.off_tiles = off;
        off = fm_align16(off + (h.n_tiles + 1) * 8);
        h.off_samples = off;
        h.n_samples = (n + s - 1) / s;
        off = fm_align16(off + h.n_samples * 4);
    }
    h.bytes = off;
}

// bytes of an index of class cls, and what a caller allocates before sigma is known
SA_HD uint64_t fm_class_bytes(uint64_t n, uint32_t cls, uint32_t s) {
    FmHeader h;
    fm_layout(h, n, cls, s);
    return h.bytes;
}
SA_HD uint64_t fm_index_bytes(uint64_t n, uint32_t s) {
    uint64_t m = 0;
    for (uint32_t k = 0; k < kFmClasses; ++k) {
        const uint64_t b = fm_class_bytes(n, k, s);
        m = b > m ? b : m;
    }
    return m;
}

// The header of (n, p, last, the plain byte counts of the BWT, s).  n == 0: p,
// last and the counts are not looked at.
SA_HD void fm_header_fill(FmHeader& h, uint64_t n, uint64_t p, uint32_t last, const uint32_t* counts, uint32_t s) {
    memset(&h, 0, sizeof h);
    h.magic = kFmMagic;
    h.version = kFmVersion;
    h.n = n;
    h.p = n ? p : 0;
    h.last = n ? last : 0;
    uint32_t sigma = 0, run = 0;
    for (uint32_t c = 0; c < 256; ++c) {
        const uint32_t k = n ? counts[c] : 0u;
        h.col[c] = (uint16_t)(k ? sigma++ : kFmAbsent);
        h.C[c] = run;
        h.base[c] = run + ((n && c == last) ? 1u : 0u);
        run += k;
    }
    h.C[256] = run;
    h.sigma = sigma;
    fm_layout(h, n, fm_class(sigma), s);
}

// ---- a checked index ------------------------------------------------------------
struct FmView {
    const uint8_t* blocks;
    const uint64_t* words;
    const uint32_t* wcnt;
    const uint64_t* tiles;
    const uint32_t* samples;
    const uint16_t* col;
    const uint32_t* C;
    const uint32_t* base;
    uint64_t n, n_samples;
    uint32_t p, last, cls, cols, rows, rec, s;
    // ibwt_dir_index's directory
    SA_HD uint64_t word(uint32_t w) const { return words[w]; }
    SA_HD uint64_t count(uint32_t w) const { return wcnt[w]; }
    SA_HD uint64_t tile(uint32_t t) const { return tiles[t]; }
};

// The header check: h is the first sizeof(FmHeader) bytes of the index_bytes at
// idx (the caller has seen that index_bytes >= kFmHeaderBytes).  True: every
// section lies where fm_layout puts it for the header's (n, class, s) and ends
// inside index_bytes, so v's arrays can be indexed by any row <= n (blocks: row /
// rows), any word < ceil(n / 64) and any sample < n_samples.  The tables (col, C,
// base) and the sections' contents are not checked: their values are clamped
// where they are used.
SA_HD bool fm_view(const FmHeader& h, const uint8_t* idx, uint64_t index_bytes, FmView& v) {
    if (index_bytes < kFmHeaderBytes || h.magic != kFmMagic || h.version != kFmVersion) return false;
    if (h.n > 0xFFFFFFFFull || h.cls >= kFmClasses || h.sample > kFmMaxSample || h.last > 255u) return false;
    if (h.n ? h.p >= h.n : h.p != 0) return false;
    FmHeader g;
    fm_layout(g, h.n, h.cls, h.sample);
    if (g.bytes > index_bytes || h.bytes != g.bytes || h.cols != g.cols || h.rows != g.rows || h.rec != g.rec ||
        h.off_blocks != g.off_blocks || h.n_blocks != g.n_blocks || h.off_words != g.off_words ||
        h.n_words != g.n_words || h.off_wcnt != g.off_wcnt || h.off_tiles != g.off_tiles || h.n_tiles != g.n_tiles ||
        h.off_samples != g.off_samples || h.n_samples != g.n_samples)
        return false;
    v.blocks = idx + g.off_blocks;
    v.words = reinterpret_cast<const uint64_t*>(idx + g.off_words);
    v.wcnt = reinterpret_cast<const uint32_t*>(idx + g.off_wcnt);
    v.tiles = reinterpret_cast<const uint64_t*>(idx + g.off_tiles);
    v.samples = reinterpret_cast<const uint32_t*>(idx + g.off_samples);
    v.col = reinterpret_cast<const uint16_t*>(idx + offsetof(FmHeader, col));
    v.C = reinterpret_cast<const uint32_t*>(idx + offsetof(FmHeader, C));
    v.base = reinterpret_cast<const uint32_t*>(idx + offsetof(FmHeader, base));
    v.n = h.n;
    v.n_samples = g.n_samples;
    v.p = (uint32_t)h.p;
    v.last = h.last;
    v.cls = g.cls;
    v.cols = g.cols;
    v.rows = g.rows;
    v.rec = g.rec;
    v.s = g.sample;
    return true;
}

// ---- occ ------------------------------------------------------------------------
// record b, b <= n / rows
SA_HD const uint8_t* fm_record(const FmView& v, uint64_t b) { return v.blocks + b * v.rec; }
SA_HD const uint8_t* fm_payload(const FmView& v, uint64_t b) { return fm_record(v, b) + v.cols * 4u; }

// the bytes of piece g (kFmPiece bytes each) of a block that lie below its row `rem`
SA_HD uint32_t fm_piece_len(uint32_t rem, uint32_t g) {
    const uint32_t a = g * kFmPiece;
    return rem <= a ? 0u : (rem - a < kFmPiece ? rem - a : kFmPiece);
}

// 0x80 in every byte of w that equals c (exact: no carry crosses a byte)
SA_HD uint64_t fm_eq_bytes(uint64_t w, uint32_t c) {
    const uint64_t k7 = 0x7F7F7F7F7F7F7F7Full;
    const uint64_t x = w ^ (0x0101010101010101ull * (uint64_t)(c & 255u));
    return ~(((x & k7) + k7) | x | k7);
}

// the bytes equal to c among the first len <= kFmPiece of a piece; ld(k) = its
// little-endian 8 bytes from byte 8 k.  Only the words that hold one of the len
// bytes are loaded, the last one under a mask.
template <class Ld>
SA_HD uint32_t fm_count_eq(const Ld& ld, uint32_t len, uint32_t c) {
    uint32_t cnt = 0;
    for (uint32_t k = 0; 8u * k < len; ++k) {
        const uint32_t left = len - 8u * k;
        const uint64_t mask = left >= 8u ? ~0ull : (1ull << (8u * left)) - 1ull;
        cnt += (uint32_t)__builtin_popcountll(fm_eq_bytes(ld(k), c) & mask);
    }
    return cnt;
}

// occ(c, r) for r <= n and the column j < cols of c, by one caller
SA_HD uint32_t fm_occ(const FmView& v, uint32_t c, uint32_t j, uint64_t r) {
    const uint64_t b = r / v.rows;
    const uint32_t rem = (uint32_t)(r % v.rows);
    const uint8_t* pl = fm_payload(v, b);
    uint32_t cnt;
    memcpy(&cnt, fm_record(v, b) + 4u * j, 4);
    for (uint32_t g = 0; g * kFmPiece < rem; ++g)
        cnt += fm_count_eq([&](uint32_t k) {
            uint64_t w;
            memcpy(&w, pl + g * kFmPiece + 8u * k, 8);
            return w;
        }, fm_piece_len(rem, g), c);
    return cnt;
}

// the column of byte c, kFmAbsent when the text lacks it (or the table is not one)
SA_HD uint32_t fm_col(const FmView& v, uint32_t c) {
    const uint32_t j = v.col[c & 255u];
    return j < v.cols ? j : kFmAbsent;
}
SA_HD uint32_t fm_clamp(uint64_t x, uint64_t n) { return (uint32_t)(x < n ? x : n); }

// base[c] + occ'(c, r) from occ(c, r), clamped to n
SA_HD uint32_t fm_step_row(const FmView& v, uint32_t c, uint64_t r, uint32_t occ) {
    const uint64_t x = (uint64_t)v.base[c] + occ - ((c == v.last && r > v.p && occ) ? 1u : 0u);
    return fm_clamp(x, v.n);
}

// Backward search of the m bytes pat(0) .. pat(m - 1); occ(c, j, r) as fm_occ.
// At most m - 1 steps of two occ each, whatever the index holds.
template <class Pat, class Occ>
SA_HD void fm_search(const FmView& v, const Pat& pat, uint64_t m, const Occ& occ, uint32_t& lo, uint32_t& hi) {
    lo = 0;
    hi = (uint32_t)v.n;
    if (m == 0) return;
    uint32_t c = pat(m - 1);
    lo = fm_clamp(v.C[c], v.n);
    hi = fm_clamp(v.C[c + 1], v.n);
    for (uint64_t i = m - 1; i > 0 && lo < hi; --i) {
        c = pat(i - 1);
        const uint32_t j = fm_col(v, c);
        if (j == kFmAbsent) {
            lo = hi = 0;
            break;
        }
        lo = fm_step_row(v, c, lo, occ(c, j, lo));
        hi = fm_step_row(v, c, hi, occ(c, j, hi));
    }
    if (lo >= hi) lo = hi = 0;
}

// ---- locate ---------------------------------------------------------------------
SA_HD bool fm_marked(const FmView& v, uint32_t r) { return (v.words[r / kIbwtWordRanks] >> (r % kIbwtWordRanks)) & 1ull; }
SA_HD uint32_t fm_bwt_byte(const FmView& v, uint32_t r) { return fm_payload(v, r / v.rows)[r % v.rows]; }

// SA[r] of row r < n (an index with s > 0, n > 0): the walk, at most s steps,
// the result below n whatever the index holds
template <class Occ>
SA_HD uint32_t fm_locate_row(const FmView& v, uint32_t r, const Occ& occ) {
    uint32_t q = r, k = 0;
    while (!fm_marked(v, q) && k < v.s) {
        const uint32_t c = fm_bwt_byte(v, q);
        uint32_t j = fm_col(v, c);
        if (j == kFmAbsent) j = 0;
        const uint32_t x = fm_step_row(v, c, q, occ(c, j, q));
        q = x < v.n ? x : (uint32_t)(v.n - 1);
        ++k;
    }
    uint64_t i = ibwt_dir_index<kIbwtTileWords>(v, q);
    if (i >= v.n_samples) i = v.n_samples - 1;
    const uint64_t pos = (uint64_t)v.s * v.samples[i] + k;
    return (uint32_t)(pos < v.n ? pos : v.n - 1);
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

#include "sa_kernels.h"

namespace sa {

static_assert(SA_FM_INFO == kFmInfo && SA_FM_MAX_SAMPLE == kFmMaxSample, "sa_hip.h states them");
constexpr uint32_t kFmTileCounters = 2048;             // blocks x cols of a tile of kLfTile rows, in every class
constexpr uint64_t kFmMaxGrid = 256 * 8;               // 8 workgroups of 256 lanes fill a CU
static_assert(kLfTile / 64 * 4 == kFmTileCounters && kLfTile / 256 * 16 == kFmTileCounters &&
              kLfTile / 4096 * 256 == kFmTileCounters, "one LDS table serves the three classes");

typedef uint32_t fm_u32x4 __attribute__((ext_vector_type(4)));

// the view of the index at idx; false: not one
__device__ __forceinline__ bool fm_view_dev(const void* idx, uint64_t index_bytes, FmView& v) {
    if (index_bytes < kFmHeaderBytes) return false;
    return fm_view(*reinterpret_cast<const FmHeader*>(idx), reinterpret_cast<const uint8_t*>(idx), index_bytes, v);
}

// occ(c, r) by the G lanes of a group (lane g of it scans piece g), r <= n, j < cols: every lane gets the sum
template <uint32_t G>
__device__ __forceinline__ uint32_t fm_occ_group(const FmView& v, uint32_t c, uint32_t j, uint64_t r, uint32_t g) {
    const uint64_t b = r / v.rows;
    const uint32_t len = fm_piece_len((uint32_t)(r % v.rows), g);
    uint32_t cnt = 0;
    if (len) {
        const fm_u32x4* pl = reinterpret_cast<const fm_u32x4*>(fm_payload(v, b) + g * kFmPiece);
        uint64_t w[8];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            fm_u32x4 x = {0u, 0u, 0u, 0u};
            if (16u * k < len) x = pl[k];
            w[2 * k] = ((uint64_t)x.y << 32) | x.x;
            w[2 * k + 1] = ((uint64_t)x.w << 32) | x.z;
        }
        cnt = fm_count_eq([&](uint32_t k) { return w[k]; }, len, c);
    }
#pragma unroll
    for (uint32_t o = G / 2; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, (int)o, kWave);
    return cnt + reinterpret_cast<const uint32_t*>(fm_record(v, b))[j];
}

// ---- build ----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_fm_header(FmHeader h, uint8_t* __restrict__ idx) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&h);
    uint32_t* dst = reinterpret_cast<uint32_t*>(idx);
    for (uint32_t i = threadIdx.x; i < kFmHeaderBytes / 4; i += kBlock) dst[i] = i < sizeof(FmHeader) / 4 ? src[i] : 0u;
}

// One workgroup per tile of kLfTile rows (tiles = n / kLfTile + 1, so that the
// record n / R has its workgroup).  cnt: k_lf_scan's table, row p apart; col:
// the header's.  Writes the records of the tile's blocks, counts and payload.
__global__ __launch_bounds__(kBlock) void k_fm_records(const uint8_t* __restrict__ bwt, uint64_t n, uint64_t p,
                                                       uint32_t aligned, const uint32_t* __restrict__ cnt,
                                                       uint32_t tiles, const uint16_t* __restrict__ col, uint32_t cls,
                                                       uint8_t* __restrict__ blocks, uint64_t n_blocks) {
    __shared__ uint32_t s_cnt[kFmTileCounters];
    __shared__ uint32_t s_col[256];
    __shared__ uint32_t s_byte[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t cols = fm_cols(cls), rows = fm_rows(cls), rec = fm_record_bytes(cls);
    const uint64_t t0 = (uint64_t)blockIdx.x * kLfTile;
    const uint32_t last = bwt[p];
    for (uint32_t i = tid; i < kFmTileCounters; i += kBlock) s_cnt[i] = 0u;
    s_byte[tid] = kFmAbsent;
    __syncthreads();
    {
        const uint32_t j = col[tid];
        s_col[tid] = j < cols ? j : kFmAbsent;
        if (j < cols) s_byte[j] = tid;
    }
    __syncthreads();
    // the rows of every block and column, row p with them
    for (uint32_t d = tid; d < kLfTile / 4; d += kBlock) {
        const uint64_t r = t0 + 4ull * d;
        if (r >= n) break;
        const uint32_t w = lf_load4(bwt, r, n, aligned != 0);
        const uint32_t b = (4u * d) / rows;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t j = s_col[(w >> (8u * k)) & 255u];
            if (r + k < n && j != kFmAbsent) atomicAdd(&s_cnt[b * cols + j], 1u);
        }
    }
    __syncthreads();
    // exclusive sums over the tile's blocks, a lane per column
    if (tid < cols) {
        uint32_t run = 0;
        for (uint32_t b = 0; b < kLfTile / rows; ++b) {
            const uint32_t y = s_cnt[b * cols + tid];
            s_cnt[b * cols + tid] = run;
            run += y;
        }
    }
    __syncthreads();
    const uint64_t b0 = t0 / rows;
    for (uint32_t i = tid; i < kFmTileCounters; i += kBlock) {
        const uint64_t gb = b0 + i / cols;
        const uint32_t j = i % cols, c = s_byte[j];
        if (gb >= n_blocks) continue;
        uint32_t x = 0;
        if (c != kFmAbsent) x = cnt[(uint64_t)c * tiles + blockIdx.x] + s_cnt[i] + ((c == last && p < t0) ? 1u : 0u);
        reinterpret_cast<uint32_t*>(blocks + gb * rec)[j] = x;
    }
    for (uint32_t d = tid; d < kLfTile / 4; d += kBlock) {
        const uint64_t r = t0 + 4ull * d;
        const uint64_t gb = r / rows;
        if (gb >= n_blocks) break;
        *reinterpret_cast<uint32_t*>(blocks + gb * rec + cols * 4u + (uint32_t)(r % rows)) =
            lf_load4(bwt, r, n, aligned != 0);
    }
}

// the mark word of this lane: word threadIdx.x of tile blockIdx.x (wavefront w takes its 64 words in turn, a
// ballot each over 64 coalesced SA entries); emit(row, sa, ballot) for every marked row when asked
template <class Emit>
__device__ __forceinline__ uint64_t fm_mark_words(const uint32_t* __restrict__ sa, uint64_t n, uint32_t s,
                                                  const Emit& emit) {
    const uint32_t lane = lane_id();
    const uint64_t w0 = (uint64_t)blockIdx.x * kIbwtTileWords + wave_id() * kWave;
    uint64_t mine = 0;
    for (uint32_t i = 0; i < (uint32_t)kWave; ++i) {
        const uint64_t r = (w0 + i) * kIbwtWordRanks + lane;
        if ((w0 + i) * kIbwtWordRanks >= n) break;   // uniform
        const uint32_t x = r < n ? sa[r] : 1u;
        const bool mark = r < n && x % s == 0u;
        const uint64_t m = __ballot(mark);
        if (lane == i) mine = m;
        if (mark) emit(w0 + i, x, m);
    }
    return mine;
}

// tex[t + 1] = the marks of tile t (summed afterwards), tex[0] = 0
__global__ __launch_bounds__(kBlock) void k_fm_marks(const uint32_t* __restrict__ sa, uint64_t n, uint32_t s,
                                                     uint64_t* __restrict__ words, uint32_t* __restrict__ wcnt,
                                                     uint64_t* __restrict__ tex) {
    __shared__ uint32_t s_w[kWaves];
    const uint64_t m = fm_mark_words(sa, n, s, [](uint64_t, uint32_t, uint64_t) {});
    const uint64_t w = (uint64_t)blockIdx.x * kIbwtTileWords + threadIdx.x;
    uint32_t sum;
    const uint32_t before = mem_block_excl((uint32_t)__popcll(m), s_w, sum);
    words[w] = m;
    wcnt[w] = before;
    if (threadIdx.x == 0) {
        tex[blockIdx.x + 1] = sum;
        if (blockIdx.x == 0) tex[0] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_fm_samples(const uint32_t* __restrict__ sa, uint64_t n, uint32_t s,
                                                       const uint32_t* __restrict__ wcnt,
                                                       const uint64_t* __restrict__ tex,
                                                       uint32_t* __restrict__ samples, uint64_t n_samples) {
    const uint64_t t = tex[blockIdx.x];
    const uint64_t lt = lanemask_lt();
    (void)fm_mark_words(sa, n, s, [&](uint64_t w, uint32_t x, uint64_t m) {
        const uint64_t i = t + wcnt[w] + (uint64_t)__popcll(m & lt);
        if (i < n_samples) samples[i] = x / s;
    });
}

// the checks of sa_fm_build_device, all before any HIP call
static int fm_build_check(const sa_context* c, const uint8_t* d_bwt, uint64_t n, uint64_t primary, const uint32_t* d_sa,
                          uint32_t s, const void* d_index, uint64_t index_bytes) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (s > kFmMaxSample) return set_err(SA_E_INVALID, "sa_sample %u is above %u", s, kFmMaxSample);
    if (!d_index) return set_err(SA_E_INVALID, "d_index is NULL");
    if ((uintptr_t)d_index & 15u) return set_err(SA_E_INVALID, "d_index is not 16-byte aligned");
    if (index_bytes < fm_index_bytes(n, s))
        return set_err(SA_E_INVALID, "index_bytes %llu is below sa_fm_index_bytes = %llu", (unsigned long long)index_bytes,
                       (unsigned long long)fm_index_bytes(n, s));
    if (n == 0) return SA_OK;
    if (!d_bwt) return set_err(SA_E_INVALID, "d_bwt is NULL");
    if (primary >= n) return set_err(SA_E_INVALID, "primary index %llu is not below n", (unsigned long long)primary);
    if (s && !d_sa) return set_err(SA_E_INVALID, "d_sa is NULL with sa_sample %u", s);
    if (!s && d_sa) return set_err(SA_E_INVALID, "d_sa is given with sa_sample 0");
    if ((uintptr_t)d_sa & 3u) return set_err(SA_E_INVALID, "d_sa is not 4-byte aligned");
    return check_no_alias({d_index}, {d_bwt, d_sa}, "d_index may not alias d_bwt or d_sa");
}

static void fm_info_out(const FmHeader& h, uint64_t* info) {
    if (!info) return;
    info[0] = h.sigma;
    info[1] = h.cls;
    info[2] = h.bytes;
    info[3] = h.n_samples;
}

// Host waits: one, for the byte totals (sigma decides the class).
static int fm_build_device(sa_context* c, const uint8_t* d_bwt, uint64_t n, uint64_t primary, const uint32_t* d_sa,
                           uint32_t s, void* d_index, uint64_t index_bytes, uint64_t* info, hipStream_t st) {
    SA_TRY(fm_build_check(c, d_bwt, n, primary, d_sa, s, d_index, index_bytes));
    SA_HIP(hipSetDevice(c->device));
    uint8_t* idx = (uint8_t*)d_index;
    FmHeader h;
    if (n == 0) {
        fm_header_fill(h, 0, 0, 0, nullptr, s);
        SA_HIP(hipMemsetAsync(idx, 0, h.bytes, st));   // the one record and the directory's tex[0]
        hipLaunchKernelGGL(k_fm_header, dim3(1), dim3(kBlock), 0, st, h, idx);
        SA_HIP(hipGetLastError());
        fm_info_out(h, info);
        return SA_OK;
    }
    const uint32_t tiles = (uint32_t)(n / kLfTile + 1);   // <= 2^17 + 1
    LocBuf tmp;
    SA_TRY(tmp.alloc(((uint64_t)tiles * 256 + 256) * 4, st));
    uint32_t* d_cnt = (uint32_t*)tmp.p;
    uint32_t* d_tot = d_cnt + (uint64_t)tiles * 256;
    const uint32_t aligned = ((uintptr_t)d_bwt & 3u) == 0u;
    hipLaunchKernelGGL(k_lf_hist, dim3(tiles), dim3(kLfBlock), 0, st, d_bwt, n, primary, aligned, d_cnt, tiles);
    hipLaunchKernelGGL(k_lf_scan, dim3(256), dim3(kBlock), 0, st, d_cnt, tiles, d_tot);
    SA_HIP(hipGetLastError());
    static_assert(hw(kHwFmTotals).len == 257, "256 totals and bwt[p]");
    uint32_t* hw = c->host_words + sa::hw(kHwFmTotals).at;
    hw[256] = 0;
    SA_HIP(hipMemcpyAsync(hw, d_tot, 256 * 4, hipMemcpyDeviceToHost, st));
    SA_HIP(hipMemcpyAsync(hw + 256, d_bwt + primary, 1, hipMemcpyDeviceToHost, st));
    SA_HIP(host_sync(st));
    const uint32_t last = hw[256] & 255u;
    uint32_t counts[256];
    for (uint32_t k = 0; k < 256; ++k) counts[k] = hw[k] + (k == last ? 1u : 0u);   // the table leaves row p out
    fm_header_fill(h, n, primary, last, counts, s);
    SA_TRACE("fm: sigma %u class %u, %llu bytes, %llu samples", h.sigma, h.cls, (unsigned long long)h.bytes,
             (unsigned long long)h.n_samples);
    if (h.C[256] != n) return set_err(SA_E_INTERNAL, "fm: the byte counts sum to %u of %llu", h.C[256], (unsigned long long)n);
    hipLaunchKernelGGL(k_fm_header, dim3(1), dim3(kBlock), 0, st, h, idx);
    hipLaunchKernelGGL(k_fm_records, dim3(tiles), dim3(kBlock), 0, st, d_bwt, n, primary, aligned, (const uint32_t*)d_cnt,
                       tiles, reinterpret_cast<const uint16_t*>(idx + offsetof(FmHeader, col)), h.cls,
                       idx + h.off_blocks, h.n_blocks);
    SA_HIP(hipGetLastError());
    if (s) {
        uint64_t* d_tex = reinterpret_cast<uint64_t*>(idx + h.off_tiles);
        SA_HIP(hipMemsetAsync(d_tex, 0, h.bytes - h.off_tiles, st));   // the sections' padding, and samples an SA that is none leaves out
        uint32_t* d_wcnt = reinterpret_cast<uint32_t*>(idx + h.off_wcnt);
        hipLaunchKernelGGL(k_fm_marks, dim3((uint32_t)h.n_tiles), dim3(kBlock), 0, st, d_sa, n, s,
                           reinterpret_cast<uint64_t*>(idx + h.off_words), d_wcnt, d_tex);
        SA_HIP(hipGetLastError());
        SA_TRY(scan_i64<ScanSum>(reinterpret_cast<int64_t*>(d_tex + 1), h.n_tiles, st));
        hipLaunchKernelGGL(k_fm_samples, dim3((uint32_t)h.n_tiles), dim3(kBlock), 0, st, d_sa, n, s,
                           (const uint32_t*)d_wcnt, (const uint64_t*)d_tex,
                           reinterpret_cast<uint32_t*>(idx + h.off_samples), h.n_samples);
        SA_HIP(hipGetLastError());
    }
    fm_info_out(h, info);
    return SA_OK;
}

// ---- count ----------------------------------------------------------------------
// G lanes per query; the kernel of another class than the index's returns at
// once, and G == 1 answers (0, 0) everywhere for what is no index.
template <uint32_t G>
__global__ __launch_bounds__(kBlock) void k_fm_count(const void* __restrict__ idx, uint64_t index_bytes,
                                                     const uint8_t* __restrict__ pat, uint64_t pat_bytes,
                                                     const uint64_t* __restrict__ off, uint64_t nq,
                                                     uint32_t* __restrict__ lo_out, uint32_t* __restrict__ hi_out) {
    FmView v;
    const bool ok = fm_view_dev(idx, index_bytes, v);
    if (!ok) {
        if (G == 1)
            for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock)
                lo_out[q] = hi_out[q] = 0u;
        return;
    }
    if (fm_lanes(v.cls) != G) return;
    const uint32_t g = threadIdx.x % G;
    for (uint64_t q = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / G; q < nq; q += (uint64_t)gridDim.x * (kBlock / G)) {
        uint64_t pa, m;
        find_pattern(off, q, pat_bytes, pa, m);
        uint32_t lo, hi;
        fm_search(v, [&](uint64_t i) { return (uint32_t)pat[pa + i]; }, m,
                  [&](uint32_t c, uint32_t j, uint64_t r) { return fm_occ_group<G>(v, c, j, r, g); }, lo, hi);
        if (g == 0) {
            lo_out[q] = lo;
            hi_out[q] = hi;
        }
    }
}

template <uint32_t G>
static uint32_t fm_grid(uint64_t items) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items * G + kBlock - 1) / kBlock, kFmMaxGrid));
}

// Host waits: none.
static int fm_count_device(const void* d_index, uint64_t index_bytes, const uint8_t* d_pat, uint64_t pat_bytes,
                           const uint64_t* d_off, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi, hipStream_t s) {
    if (nq == 0) return SA_OK;
    if (!d_index || !d_pat || !d_off || !d_lo || !d_hi) return set_err(SA_E_INVALID, "NULL device pointer");
    if ((uintptr_t)d_index & 15u) return set_err(SA_E_INVALID, "d_index is not 16-byte aligned");
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    hipLaunchKernelGGL((k_fm_count<1>), dim3(fm_grid<1>(nq)), dim3(kBlock), 0, s, d_index, index_bytes, d_pat, pat_bytes,
                       d_off, nq, d_lo, d_hi);
    hipLaunchKernelGGL((k_fm_count<4>), dim3(fm_grid<4>(nq)), dim3(kBlock), 0, s, d_index, index_bytes, d_pat, pat_bytes,
                       d_off, nq, d_lo, d_hi);
    hipLaunchKernelGGL((k_fm_count<64>), dim3(fm_grid<64>(nq)), dim3(kBlock), 0, s, d_index, index_bytes, d_pat, pat_bytes,
                       d_off, nq, d_lo, d_hi);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// ---- locate ---------------------------------------------------------------------
// c[q] into off[q + 1] (summed afterwards); words: [0] 1 for an index, [1] s, [2] n, [3] the class
__global__ __launch_bounds__(kBlock) void k_fm_loc_count(const void* __restrict__ idx, uint64_t index_bytes,
                                                         const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                         uint64_t nq, uint64_t max_hits, uint64_t* __restrict__ off,
                                                         unsigned long long* __restrict__ words) {
    FmView v;
    const bool ok = fm_view_dev(idx, index_bytes, v);
    const uint64_t n = ok ? v.n : 0;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock)
        off[q + 1] = locate_count(lo[q], hi[q], n, max_hits);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        off[0] = 0;
        words[0] = ok ? 1ull : 0ull;
        words[1] = ok ? v.s : 0ull;
        words[2] = n;
        words[3] = ok ? v.cls : 0ull;
    }
}

// hit e of the batch: row lo[q] + (e - off[q]) of its query q, resolved by the group's G lanes into out[e]
template <uint32_t G>
__global__ __launch_bounds__(kBlock) void k_fm_resolve(const void* __restrict__ idx, uint64_t index_bytes,
                                                       const uint32_t* __restrict__ lo, uint64_t nq,
                                                       const uint64_t* __restrict__ off, uint64_t total,
                                                       uint32_t* __restrict__ out) {
    FmView v;
    if (!fm_view_dev(idx, index_bytes, v) || fm_lanes(v.cls) != G || v.s == 0 || v.n == 0) return;
    const uint32_t g = threadIdx.x % G;
    for (uint64_t e = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / G; e < total; e += (uint64_t)gridDim.x * (kBlock / G)) {
        const uint64_t q = locate_lower_bound(LocOff{off}, 0, nq, e + 1) - 1;   // off[q] <= e < off[q + 1]
        const uint64_t r = std::min<uint64_t>((uint64_t)lo[q] + (e - off[q]), v.n - 1);
        const uint32_t pos = fm_locate_row(v, (uint32_t)r, [&](uint32_t c, uint32_t j, uint64_t x) {
            return fm_occ_group<G>(v, c, j, x, g);
        });
        if (g == 0) out[e] = pos;
    }
}

// the checks of sa_fm_locate_device, all before any HIP call
static int fm_locate_check(const sa_context* c, const void* d_index, const uint32_t* d_lo, const uint32_t* d_hi,
                           uint64_t nq, uint32_t flags, const uint64_t* d_off, const uint64_t* total) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!total) return set_err(SA_E_INVALID, "total is NULL");
    if (!d_index) return set_err(SA_E_INVALID, "d_index is NULL");
    if ((uintptr_t)d_index & 15u) return set_err(SA_E_INVALID, "d_index is not 16-byte aligned");
    if (!d_lo) return set_err(SA_E_INVALID, "d_lo is NULL");
    if (!d_hi) return set_err(SA_E_INVALID, "d_hi is NULL");
    if (!d_off) return set_err(SA_E_INVALID, "d_off is NULL");
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    return check_flags(flags, SA_LOCATE_SA_ORDER | SA_LOCATE_SMALL_CHUNKS);
}

// Host waits: one for the total and the header's words; then sa_locate_device's
// own over the materialised hits, or one at the end in SA order.
static int fm_locate_device(sa_context* c, const void* d_index, uint64_t index_bytes, const uint32_t* d_lo,
                            const uint32_t* d_hi, uint64_t nq, uint64_t max_hits, uint32_t flags, uint64_t* d_off,
                            uint32_t* d_pos, uint64_t pos_cap, uint64_t* total, hipStream_t s) {
    SA_TRY(fm_locate_check(c, d_index, d_lo, d_hi, nq, flags, d_off, total));
    *total = 0;
    SA_HIP(hipSetDevice(c->device));
    uint64_t* h = host_u64<kHwFmLocate, 5>(c);
    {
        LocBuf w;
        SA_TRY(w.alloc(32, s));
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nq + kBlock - 1) / kBlock, (uint64_t)c->cus * 8));
        hipLaunchKernelGGL(k_fm_loc_count, dim3(grid), dim3(kBlock), 0, s, d_index, index_bytes, d_lo, d_hi, nq, max_hits,
                           d_off, (unsigned long long*)w.p);
        SA_HIP(hipGetLastError());
        if (nq) SA_TRY(scan_i64<ScanSum>(reinterpret_cast<int64_t*>(d_off) + 1, nq, s));
        SA_HIP(hipMemcpyAsync(h, w.p, 32, hipMemcpyDeviceToHost, s));
        SA_HIP(hipMemcpyAsync(h + 4, d_off + nq, 8, hipMemcpyDeviceToHost, s));
    }
    SA_HIP(host_sync(s));
    const uint64_t sum = h[4], n = h[2];
    const uint32_t cls = (uint32_t)h[3];
    SA_TRACE("fm locate: nq %llu total %llu (index %llu, s %llu, n %llu)", (unsigned long long)nq, (unsigned long long)sum,
             (unsigned long long)h[0], (unsigned long long)h[1], (unsigned long long)n);
    if (!h[0]) return set_err(SA_E_INVALID, "not an FM-index");
    if (!h[1]) return set_err(SA_E_INVALID, "no samples: the index was built with sa_sample 0");
    if (sum > 0xFFFFFFFFull)
        return set_err(SA_E_INVALID, "%llu hits are more than 2^32 - 1: cap it with max_hits", (unsigned long long)sum);
    *total = sum;
    if (!d_pos || sum > pos_cap || sum == 0) return SA_OK;
    const bool direct = (flags & SA_LOCATE_SA_ORDER) != 0;
    ListSort tmp;   // the hits resolved in SA order, then sorted
    if (!direct) SA_TRY(tmp.alloc(sum, nq, s));
    uint32_t* d_hits = direct ? d_pos : tmp.items;
    if (cls == 0)
        hipLaunchKernelGGL((k_fm_resolve<1>), dim3(fm_grid<1>(sum)), dim3(kBlock), 0, s, d_index, index_bytes, d_lo, nq,
                           (const uint64_t*)d_off, sum, d_hits);
    else if (cls == 1)
        hipLaunchKernelGGL((k_fm_resolve<4>), dim3(fm_grid<4>(sum)), dim3(kBlock), 0, s, d_index, index_bytes, d_lo, nq,
                           (const uint64_t*)d_off, sum, d_hits);
    else
        hipLaunchKernelGGL((k_fm_resolve<64>), dim3(fm_grid<64>(sum)), dim3(kBlock), 0, s, d_index, index_bytes, d_lo, nq,
                           (const uint64_t*)d_off, sum, d_hits);
    SA_HIP(hipGetLastError());
    if (direct) {
        SA_HIP(host_sync(s));
        return SA_OK;
    }
    // the hits as an SA of their own, sorted list by list
    return tmp.sort(c, "fm locate", "hits", sum, nq, flags, d_off, d_pos, pos_cap, n, s);
}

// ---- host in, host out, over the steps of sa_host.h -----------------------------
static int fm_build_host(const uint8_t* bwt, uint64_t n, uint64_t primary, const void* sa, int sa_width, uint32_t s,
                         void* index_out, uint64_t index_bytes, uint64_t* info) {
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (s > kFmMaxSample) return set_err(SA_E_INVALID, "sa_sample %u is above %u", s, kFmMaxSample);
    if (!index_out) return set_err(SA_E_INVALID, "index_out is NULL");
    if (index_bytes < fm_index_bytes(n, s))
        return set_err(SA_E_INVALID, "index_bytes %llu is below sa_fm_index_bytes = %llu", (unsigned long long)index_bytes,
                       (unsigned long long)fm_index_bytes(n, s));
    if (n == 0) {   // the empty index is the host's own: a header, one record of zeros, the directory's first sum
        FmHeader h;
        fm_header_fill(h, 0, 0, 0, nullptr, s);
        memset(index_out, 0, h.bytes);
        memcpy(index_out, &h, sizeof h);
        fm_info_out(h, info);
        return SA_OK;
    }
    if (!bwt) return set_err(SA_E_INVALID, "NULL host pointer");
    if (primary >= n) return set_err(SA_E_INVALID, "primary index %llu is not below n", (unsigned long long)primary);
    if (s && !sa) return set_err(SA_E_INVALID, "sa is NULL with sa_sample %u", s);
    if (!s && sa) return set_err(SA_E_INVALID, "sa is given with sa_sample 0");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    if (s) SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_bwt, d_sa, d_idx;
    SA_TRY(d_bwt.alloc(align_up(n, 256)));
    if (s) SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_idx.alloc(index_bytes));
    SA_TRY(upload({{d_bwt.p, bwt, n}, {d_sa.p, src, s ? n * 4 : 0}}));
    uint64_t w[kFmInfo] = {0, 0, 0, 0};
    SA_TRY(fm_build_device(c, d_bwt.as<uint8_t>(), n, primary, d_sa.as<uint32_t>(), s, d_idx.p, index_bytes, w, nullptr));
    if (info) memcpy(info, w, sizeof w);
    return copy_d2h(index_out, d_idx.as<uint32_t>(), w[2] / 4, 4, nullptr);
}

// the header of a host index, checked: "not an FM-index" otherwise
static int fm_host_view(const void* index, uint64_t index_bytes, FmHeader& h, FmView& v) {
    if (!index) return set_err(SA_E_INVALID, "index is NULL");
    if (index_bytes < kFmHeaderBytes) return set_err(SA_E_INVALID, "not an FM-index: %llu bytes hold no header", (unsigned long long)index_bytes);
    memcpy(&h, index, sizeof h);
    if (!fm_view(h, (const uint8_t*)index, index_bytes, v))
        return set_err(SA_E_INVALID, "not an FM-index: the magic, the version or a section does not fit %llu bytes",
                       (unsigned long long)index_bytes);
    return SA_OK;
}

static int fm_count_host(const void* index, uint64_t index_bytes, const uint8_t* pat, const uint64_t* pat_off, uint64_t nq,
                         uint64_t* lo_out, uint64_t* hi_out) {
    FmHeader h;
    FmView v;
    SA_TRY(fm_host_view(index, index_bytes, h, v));
    if (nq == 0) return SA_OK;
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (!pat_off || !lo_out || !hi_out) return set_err(SA_E_INVALID, "NULL host pointer");
    for (uint64_t q = 0; q < nq; ++q)
        if (pat_off[q] > pat_off[q + 1]) return set_err(SA_E_INVALID, "pattern offsets decrease at %llu", (unsigned long long)q);
    const uint64_t pat_bytes = pat_off[nq];
    if (pat_bytes && !pat) return set_err(SA_E_INVALID, "NULL host pointer");
    if (h.n == 0) {   // nothing occurs in the empty text, and the empty pattern has [0, 0)
        for (uint64_t q = 0; q < nq; ++q) lo_out[q] = hi_out[q] = 0;
        return SA_OK;
    }
    SA_TRY(need_device());
    DevBuf d_idx, d_pat, d_off, d_lo, d_hi;
    SA_TRY(d_idx.alloc(h.bytes));
    SA_TRY(d_pat.alloc(align_up(pat_bytes + 1, 256)));
    SA_TRY(d_off.alloc((nq + 1) * 8));
    SA_TRY(d_lo.alloc(nq * 4));
    SA_TRY(d_hi.alloc(nq * 4));
    SA_TRY(upload({{d_idx.p, index, h.bytes}, {d_pat.p, pat, pat_bytes}, {d_off.p, pat_off, (nq + 1) * 8}}));
    SA_TRY(fm_count_device(d_idx.p, h.bytes, d_pat.as<uint8_t>(), pat_bytes, d_off.as<uint64_t>(), nq,
                           d_lo.as<uint32_t>(), d_hi.as<uint32_t>(), nullptr));
    return download_u64({{lo_out, d_lo.as<uint32_t>()}, {hi_out, d_hi.as<uint32_t>()}}, nq);
}

static int fm_locate_host(const void* index, uint64_t index_bytes, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                          uint64_t max_hits, uint32_t flags, uint64_t* off_out, void* pos_out, int pos_width,
                          uint64_t pos_cap) {
    SA_TRY(check_width(pos_width));
    FmHeader h;
    FmView v;
    SA_TRY(fm_host_view(index, index_bytes, h, v));
    if (h.sample == 0) return set_err(SA_E_INVALID, "no samples: the index was built with sa_sample 0");
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    SA_TRY(check_flags(flags, SA_LOCATE_SA_ORDER | SA_LOCATE_SMALL_CHUNKS));
    if (!off_out) return set_err(SA_E_INVALID, "off_out is NULL");
    off_out[0] = 0;
    if (nq == 0) return SA_OK;
    std::vector<uint32_t> lh;
    SA_TRY(pack_intervals(lo, hi, nq, h.n, max_hits, off_out, lh));
    const uint64_t total = off_out[nq];
    if (total > 0xFFFFFFFFull)
        return set_err(SA_E_INVALID, "%llu hits are more than 2^32 - 1: cap it with max_hits", (unsigned long long)total);
    if (pos_cap < total)
        return set_err(SA_E_INVALID, "pos_cap %llu is below the %llu hits", (unsigned long long)pos_cap,
                       (unsigned long long)total);
    if (total == 0) return SA_OK;
    if (!pos_out) return set_err(SA_E_INVALID, "pos_out is NULL");
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(std::max<uint64_t>(total, 1), &c));
    DevBuf d_idx, d_lh, d_off, d_pos;
    SA_TRY(d_idx.alloc(h.bytes));
    SA_TRY(d_lh.alloc(align_up(2 * nq, 64) * 4));
    SA_TRY(d_off.alloc(align_up(nq + 1, 64) * 8));
    SA_TRY(d_pos.alloc(align_up(total, 64) * 4));
    SA_TRY(upload({{d_idx.p, index, h.bytes}, {d_lh.p, lh.data(), 2 * nq * 4}}));
    uint64_t got = 0;
    SA_TRY(fm_locate_device(c, d_idx.p, h.bytes, d_lh.as<uint32_t>(), d_lh.as<uint32_t>() + nq, nq, max_hits, flags,
                            d_off.as<uint64_t>(), d_pos.as<uint32_t>(), total, &got, nullptr));
    if (got != total)
        return set_err(SA_E_INTERNAL, "fm locate: the device counted %llu hits, the host %llu", (unsigned long long)got,
                       (unsigned long long)total);
    return copy_d2h(pos_out, d_pos.as<uint32_t>(), total, pos_width, nullptr);
}

}  // namespace sa

extern "C" {

uint64_t sa_fm_index_bytes(uint64_t n, uint32_t sa_sample) { return sa::fm_index_bytes(n, sa_sample); }

int sa_fm_build_device(sa_context* ctx, const uint8_t* d_bwt, uint64_t n, uint64_t primary, const uint32_t* d_sa,
                       uint32_t sa_sample, void* d_index, uint64_t index_bytes, uint64_t* info, void* stream) {
    return sa::fm_build_device(ctx, d_bwt, n, primary, d_sa, sa_sample, d_index, index_bytes, info, (hipStream_t)stream);
}

int sa_fm_count_device(const void* d_index, uint64_t index_bytes, const uint8_t* d_pat, uint64_t pat_bytes,
                       const uint64_t* d_pat_off, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi, void* stream) {
    return sa::fm_count_device(d_index, index_bytes, d_pat, pat_bytes, d_pat_off, nq, d_lo, d_hi, (hipStream_t)stream);
}

int sa_fm_locate_device(sa_context* ctx, const void* d_index, uint64_t index_bytes, const uint32_t* d_lo,
                        const uint32_t* d_hi, uint64_t nq, uint64_t max_hits, uint32_t flags, uint64_t* d_off,
                        uint32_t* d_pos, uint64_t pos_cap, uint64_t* total, void* stream) {
    return sa::fm_locate_device(ctx, d_index, index_bytes, d_lo, d_hi, nq, max_hits, flags, d_off, d_pos, pos_cap, total,
                                (hipStream_t)stream);
}

int sa_fm_build(const uint8_t* bwt, uint64_t n, uint64_t primary, const void* sa, int sa_width, uint32_t sa_sample,
                void* index_out, uint64_t index_bytes, uint64_t* info) {
    return sa::fm_build_host(bwt, n, primary, sa, sa_width, sa_sample, index_out, index_bytes, info);
}

int sa_fm_count(const void* index, uint64_t index_bytes, const uint8_t* pat, const uint64_t* pat_off, uint64_t nq,
                uint64_t* lo_out, uint64_t* hi_out) {
    return sa::fm_count_host(index, index_bytes, pat, pat_off, nq, lo_out, hi_out);
}

int sa_fm_locate(const void* index, uint64_t index_bytes, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                 uint64_t max_hits, uint32_t flags, uint64_t* off_out, void* pos_out, int pos_width, uint64_t pos_cap) {
    return sa::fm_locate_host(index, index_bytes, lo, hi, nq, max_hits, flags, off_out, pos_out, pos_width, pos_cap);
}

}  // extern "C"

#endif   // __HIPCC__
