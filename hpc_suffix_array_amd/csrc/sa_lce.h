// sa_lce.h -- longest common extensions: a range-minimum index over the LCP
// array and the batched queries it answers (sa_lce_index_bytes,
// sa_lce_build_device, sa_lcp_min_device, sa_lce_device,
// sa_substr_compare_device and the host forms sa_lcp_min, sa_lce,
// sa_substr_compare of include/sa_hip.h).
//
// Definitions.  LCP follows sa_lcp_device: lcp[0] = 0, lcp[r] = lcp(SA[r - 1],
// SA[r]), n <= 2^32 - 1.  kLceNone = 0xFFFFFFFF is the minimum's identity.
//   lcp_min(lo, hi)  of an SA interval [lo, hi): min lcp[lo + 1 .. hi - 1], the
//                    length of the longest common prefix of all its suffixes
//                    (its string depth).  The empty minimum (hi - lo <= 1) is
//                    kLceNone, and so is an interval that breaks lo < hi <= n.
//   lce(i, j)        of two text positions, ISA the inverse suffix array: a
//                    position >= n is the empty suffix, lce = 0 when either is;
//                    lce(i, i) = n - i; otherwise with a = min(ISA[i], ISA[j])
//                    and b = max(ISA[i], ISA[j]) it is min lcp[a + 1 .. b].
//   order            of T[i, i + li) and T[j, j + lj), lengths clipped to the
//                    text's end: l = min(lce(i, j), li, lj); when l == min(li,
//                    lj) it is sign(li - lj), otherwise -1 when ISA[i] < ISA[j],
//                    else +1 (int8).  No text byte is needed: below both
//                    lengths, substring order is suffix order.
//
// The index is one flat byte buffer that holds offsets and never pointers (16-
// byte aligned, copyable):
//   header   kLceHeaderBytes = 4096: LceHeader (magic, version, n, the section
//            offsets), zero after it
//   blk      six levels of nb = ceil(n / 64) uint32: blk[k][b] = the minimum of
//            the blocks [b, b + 2^k) of 64 ranks each, clipped at the end of b's
//            superblock (64 blocks = 4096 ranks) and at nb
//   top      levels = floor(log2 ns) + 1 levels of ns = ceil(nb / 64) uint32:
//            top[k][s] = the minimum of the superblocks [s, s + 2^k), clipped at ns
// 4096 + 4 (6 nb + levels ns) bytes, rounded up to 16: under 0.40 n + 8 KiB for
// n >= 2^20, beside the 4 n bytes of the LCP array.
//
//   k_lce_blocks   one workgroup per superblock: 4096 LCP entries in 16-byte
//                  loads, the 64 block minima by reductions over 16 lanes, the
//                  six levels in LDS, written coalesced, plus top[0][s]
//   k_lce_top      one level of the top table from the one below it
//   k_lce_header   the header, last
//   k_lce_query    16 lanes per query, four queries per wavefront.  The
//                  inclusive rank range [x, y] is the tail of block(x), the head
//                  of block(y) (at most 256 bytes of LCP each: one 16-byte load
//                  per lane, masked to the range) and the whole blocks between
//                  them: two overlapping cells of blk when both ends share a
//                  superblock, otherwise two for the rest of the left
//                  superblock, two for the start of the right one and two of
//                  top -- at most six dwords, each loaded by its own lane.  No
//                  address depends on a loaded value, so a rank range costs one
//                  round trip and a pair of positions two (the ISA gathers
//                  first).  With a text, the position forms first compare
//                  kLceProbe = 16 bytes at i and j and answer from them when
//                  the mismatch lies inside.
//
// The kernel takes the layout from n, checks it against index_bytes and the
// header against it: where that fails every query answers kLceNone (order 0).
// Ranks read from ISA are clamped below n and cells to their section, so no
// load leaves text[0, n), isa[0, n), lcp[0, n) or index[0, index_bytes).
//
// The layout and the decomposition compile on the host: tests/cpp/lce_check.cpp
// checks them against brute force.  Measurements: DESIGN.md section 20.
// The HIP part needs sa_host.h before it.
#pragma once
#include <stdint.h>

#include "sa_search.h"   // SA_HD

namespace sa {

constexpr uint32_t kLceNone = 0xFFFFFFFFu;   // = SA_LCE_NONE
constexpr uint32_t kLceProbe = 16;           // = SA_LCE_PROBE: text bytes compared before the index is asked
constexpr uint32_t kLceBlock = 64;           // = SA_LCE_BLOCK: ranks per block
constexpr uint32_t kLceSuper = 4096;         // = SA_LCE_SUPER: ranks per superblock
constexpr uint32_t kLceGroup = 16;           // lanes per query
constexpr uint32_t kLceBlkLevels = 6;        // spans of 1 .. 32 blocks inside a superblock
constexpr uint32_t kLceHeaderBytes = 4096;
constexpr uint64_t kLceMagic = 0x31584945434c4153ull;   // "SALCEIX1"
constexpr uint32_t kLceVersion = 1;
static_assert(kLceSuper == kLceBlock * 64 && kLceBlock == kLceGroup * 4, "64 blocks; one uint4 per lane and block");

struct LceHeader {
    uint64_t magic;
    uint32_t version, levels;
    uint64_t n, nb, ns;
    uint64_t off_blk, off_top;   // bytes from the start of the index
    uint64_t bytes;              // of the whole index
};
static_assert(sizeof(LceHeader) == 64, "16 words");

SA_HD uint32_t lce_log2(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x | 1ull); }   // floor, 0 for 0

// the sections of the index of n ranks
SA_HD LceHeader lce_layout(uint64_t n) {
    LceHeader h;
    h.magic = kLceMagic;
    h.version = kLceVersion;
    h.n = n;
    h.nb = (n + kLceBlock - 1) / kLceBlock;
    h.ns = (h.nb + 63) / 64;
    h.levels = h.ns ? lce_log2(h.ns) + 1u : 0u;
    h.off_blk = kLceHeaderBytes;
    h.off_top = h.off_blk + 4ull * kLceBlkLevels * h.nb;
    h.bytes = (h.off_top + 4ull * h.levels * h.ns + 15ull) & ~15ull;
    return h;
}
SA_HD uint64_t lce_index_bytes(uint64_t n) { return lce_layout(n).bytes; }

SA_HD bool lce_header_ok(const LceHeader& h, const LceHeader& want) {
    return h.magic == want.magic && h.version == want.version && h.levels == want.levels && h.n == want.n &&
           h.nb == want.nb && h.ns == want.ns && h.off_blk == want.off_blk && h.off_top == want.off_top &&
           h.bytes == want.bytes;
}

// the rank range [x, y] (inclusive) of an SA interval [lo, hi); false: the empty minimum
SA_HD bool lce_interval_range(uint64_t lo, uint64_t hi, uint64_t n, uint64_t& x, uint64_t& y) {
    x = lo + 1;
    y = hi - 1;
    return lo < hi && hi <= n && hi - lo >= 2;
}

// The partial blocks of [x, y], x <= y: which = 0 the block of x, words [first,
// last] of it; which = 1 the block of y when it is another one.
SA_HD bool lce_partial(uint64_t x, uint64_t y, uint32_t which, uint64_t& block, uint32_t& first, uint32_t& last) {
    const uint64_t bx = x / kLceBlock, by = y / kLceBlock;
    if (which == 0) {
        block = bx;
        first = (uint32_t)(x % kLceBlock);
        last = bx == by ? (uint32_t)(y % kLceBlock) : kLceBlock - 1;
        return true;
    }
    block = by;
    first = 0;
    last = (uint32_t)(y % kLceBlock);
    return bx != by;
}

// Cell `slot` (0 .. 5) of the whole blocks strictly between block(x) and
// block(y): slots 0, 1 the left superblock's part (all of them when both ends
// share a superblock), 2, 3 the right superblock's, 4, 5 the superblocks between.
// top: the cell's table; word: its index in that table (level * entries + entry).
// False: the slot is not used.  Selects only: every lane evaluates its own slot.
SA_HD bool lce_cell(const LceHeader& lay, uint64_t x, uint64_t y, uint32_t slot, bool& top, uint64_t& word) {
    const uint64_t bx = x / kLceBlock, by = y / kLceBlock;
    top = slot >= 4;
    word = 0;
    if (by < bx + 2 || slot >= 6) return false;
    const uint64_t p = bx + 1, q = by - 1;   // the whole blocks [p, q]
    const uint64_t sp = p / 64, sq = q / 64;
    const bool second = (slot & 1u) != 0;
    if (slot < 4) {
        const bool right = slot >= 2;
        if (right && sp == sq) return false;
        const uint64_t s = right ? sq * 64 : p;
        const uint64_t e = (right || sp == sq) ? q : sp * 64 + 63;
        uint32_t k = lce_log2(e - s + 1);
        k = k < kLceBlkLevels - 1 ? k : kLceBlkLevels - 1;
        word = (uint64_t)k * lay.nb + (second ? e + 1 - (1ull << k) : s);
        return true;
    }
    if (sq < sp + 2) return false;
    const uint64_t s = sp + 1, e = sq - 1;
    const uint32_t k = lce_log2(e - s + 1);
    word = (uint64_t)k * lay.ns + (second ? e + 1 - (1ull << k) : s);
    return true;
}

// the lengths of a substring order clipped to the text's end, and the order
// once lce is known: 2 = "by suffix order"
SA_HD uint32_t lce_clip(uint64_t pos, uint64_t len, uint64_t n) {
    return pos >= n ? 0u : (uint32_t)(len < n - pos ? len : n - pos);
}
SA_HD int lce_order(uint32_t lce, uint32_t ci, uint32_t cj) {
    const uint32_t mn = ci < cj ? ci : cj;
    const uint32_t l = lce < mn ? lce : mn;
    return l == mn ? (int)(ci > cj) - (int)(ci < cj) : 2;
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

#include "sa_kernels.h"

namespace sa {

static_assert(kLceNone == SA_LCE_NONE && kLceProbe == SA_LCE_PROBE && kLceBlock == SA_LCE_BLOCK &&
                  kLceSuper == SA_LCE_SUPER,
              "the header's constants");
static_assert(kLceSuper == 16 * kBlock && kWave % kLceGroup == 0 && kLceProbe == kLceGroup,
              "four uint4 per thread and superblock; one probe byte per lane");
constexpr uint32_t kLceGrid = 4096;   // workgroups of a query grid at most (16 queries per workgroup and step)

__device__ __forceinline__ uint32_t lce_min4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return std::min(std::min(a, b), std::min(c, d));
}
// minimum over the kLceGroup lanes of a group
__device__ __forceinline__ uint32_t lce_group_min(uint32_t x) {
#pragma unroll
    for (int o = kLceGroup / 2; o > 0; o >>= 1) x = std::min(x, (uint32_t)__shfl_xor((int)x, o, kLceGroup));
    return x;
}

// One workgroup per superblock s: blk[k][64 s + b] for the blocks below nb and top[0][s].
__global__ __launch_bounds__(kBlock) void k_lce_blocks(const uint32_t* __restrict__ lcp, uint64_t n, uint64_t nb,
                                                       uint32_t* __restrict__ blk, uint32_t* __restrict__ top) {
    __shared__ uint32_t s_lvl[kLceBlkLevels][64];
    const uint64_t sb = blockIdx.x;
    const uint64_t base = sb * kLceSuper;
    uint4 v[4];
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) {
        const uint64_t w = base + 4ull * (p * kBlock + threadIdx.x);
        v[p] = make_uint4(kLceNone, kLceNone, kLceNone, kLceNone);
        if (w + 4 <= n) {
            v[p] = *reinterpret_cast<const uint4*>(lcp + w);
        } else {   // the quad that holds the end of the array
            if (w < n) v[p].x = lcp[w];
            if (w + 1 < n) v[p].y = lcp[w + 1];
            if (w + 2 < n) v[p].z = lcp[w + 2];
        }
    }
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) {
        const uint32_t m = lce_group_min(lce_min4(v[p].x, v[p].y, v[p].z, v[p].w));
        if (threadIdx.x % kLceGroup == 0) s_lvl[0][(p * kBlock + threadIdx.x) / kLceGroup] = m;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 1; k < kLceBlkLevels; ++k) {
        const uint32_t half = 1u << (k - 1), b = threadIdx.x;
        if (b < 64) s_lvl[k][b] = std::min(s_lvl[k - 1][b], b + half < 64 ? s_lvl[k - 1][b + half] : kLceNone);
        __syncthreads();
    }
    for (uint32_t c = threadIdx.x; c < kLceBlkLevels * 64; c += kBlock) {
        const uint32_t k = c / 64, b = c % 64;
        if (sb * 64 + b < nb) blk[(uint64_t)k * nb + sb * 64 + b] = s_lvl[k][b];
    }
    if (threadIdx.x == 0) top[sb] = std::min(s_lvl[kLceBlkLevels - 1][0], s_lvl[kLceBlkLevels - 1][32]);
}

// level k of the top table (half = 2^(k - 1)) from level k - 1
__global__ __launch_bounds__(kBlock) void k_lce_top(const uint32_t* __restrict__ below, uint32_t* __restrict__ level,
                                                    uint64_t ns, uint64_t half) {
    for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < ns; s += (uint64_t)gridDim.x * kBlock)
        level[s] = std::min(below[s], s + half < ns ? below[s + half] : kLceNone);
}

// the header, the zeros after it and the zeros that round the index up to 16 bytes
__global__ __launch_bounds__(kBlock) void k_lce_header(LceHeader h, uint32_t* __restrict__ index) {
    constexpr uint32_t kWords = sizeof(LceHeader) / 4;
    for (uint32_t w = kWords + threadIdx.x; w < kLceHeaderBytes / 4; w += kBlock) index[w] = 0;
    const uint64_t used = h.off_top / 4 + (uint64_t)h.levels * h.ns;   // at most 3 words below h.bytes / 4
    if (used + threadIdx.x < h.bytes / 4) index[used + threadIdx.x] = 0;
    if (threadIdx.x == 0) *reinterpret_cast<LceHeader*>(index) = h;
}

// The minimum of lcp[x .. y] (x <= y < n where `has`; kLceNone otherwise) for
// the group of this lane, lane gl of it.  blkw / topw: the two tables.  Every
// load is issued before the first is waited for.
__device__ __forceinline__ uint32_t lce_range_min(const LceHeader& lay, const uint32_t* __restrict__ lcp,
                                                  const uint32_t* __restrict__ blkw,
                                                  const uint32_t* __restrict__ topw, uint64_t x, uint64_t y, bool has,
                                                  uint32_t gl) {
    const uint64_t n = lay.n;
    uint4 v0 = make_uint4(kLceNone, kLceNone, kLceNone, kLceNone), v1 = v0;
    uint32_t c = kLceNone;
    uint64_t b0 = 0, b1 = 0;
    uint32_t f0 = 0, l0 = 0, f1 = 0, l1 = 0;
    const bool p0 = has && lce_partial(x, y, 0, b0, f0, l0);
    const bool p1 = has && lce_partial(x, y, 1, b1, f1, l1);
    const uint32_t w = gl * 4;   // this lane's words of a block
    const bool t0 = p0 && w + 3 >= f0 && w <= l0, t1 = p1 && w <= l1;
    const uint64_t g0 = b0 * kLceBlock + w, g1 = b1 * kLceBlock + w;
    if (t0) {
        if (g0 + 4 <= n) {
            v0 = *reinterpret_cast<const uint4*>(lcp + g0);
        } else {
            if (g0 < n) v0.x = lcp[g0];
            if (g0 + 1 < n) v0.y = lcp[g0 + 1];
            if (g0 + 2 < n) v0.z = lcp[g0 + 2];
        }
    }
    if (t1) {
        if (g1 + 4 <= n) {
            v1 = *reinterpret_cast<const uint4*>(lcp + g1);
        } else {
            if (g1 < n) v1.x = lcp[g1];
            if (g1 + 1 < n) v1.y = lcp[g1 + 1];
            if (g1 + 2 < n) v1.z = lcp[g1 + 2];
        }
    }
    bool top = false;
    uint64_t word = 0;
    if (has && lce_cell(lay, x, y, gl, top, word)) {
        const uint64_t cap = top ? (uint64_t)lay.levels * lay.ns : (uint64_t)kLceBlkLevels * lay.nb;   // > 0: n > 0
        c = (top ? topw : blkw)[std::min(word, cap - 1)];
    }
    uint32_t m = c;
    if (t0) {
        m = std::min(m, w >= f0 && w <= l0 ? v0.x : kLceNone);
        m = std::min(m, w + 1 >= f0 && w + 1 <= l0 ? v0.y : kLceNone);
        m = std::min(m, w + 2 >= f0 && w + 2 <= l0 ? v0.z : kLceNone);
        m = std::min(m, w + 3 >= f0 && w + 3 <= l0 ? v0.w : kLceNone);
    }
    if (t1) {
        m = std::min(m, w <= l1 ? v1.x : kLceNone);
        m = std::min(m, w + 1 <= l1 ? v1.y : kLceNone);
        m = std::min(m, w + 2 <= l1 ? v1.z : kLceNone);
        m = std::min(m, w + 3 <= l1 ? v1.w : kLceNone);
    }
    return lce_group_min(m);
}

enum LceMode : int { kLceRanks = 0, kLcePositions = 1, kLceOrder = 2 };

// qa / qb: lo / hi (kLceRanks) or i / j; la / lb: the lengths of kLceOrder.
// out: uint32 per query, int8 for kLceOrder.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_lce_query(LceHeader lay, const uint8_t* __restrict__ text,
                                                      const uint32_t* __restrict__ isa,
                                                      const uint32_t* __restrict__ lcp,
                                                      const uint8_t* __restrict__ index, uint64_t index_bytes,
                                                      const uint32_t* __restrict__ qa, const uint32_t* __restrict__ qb,
                                                      const uint32_t* __restrict__ la, const uint32_t* __restrict__ lb,
                                                      uint64_t nq, void* __restrict__ out) {
    constexpr uint32_t kPerWave = kWave / kLceGroup;
    const uint64_t n = lay.n;
    const uint32_t lane = lane_id(), gl = lane % kLceGroup, shift = lane - gl;
    // the layout is n's; the index holds it when the header says the same and index_bytes covers it
    const bool fits = index_bytes >= lay.bytes;
    LceHeader h = lay;
    if (fits) h = *reinterpret_cast<const LceHeader*>(index);
    const uint32_t* blkw = reinterpret_cast<const uint32_t*>(index + lay.off_blk);
    const uint32_t* topw = reinterpret_cast<const uint32_t*>(index + lay.off_top);
    for (uint64_t qw = ((uint64_t)blockIdx.x * kWaves + wave_id()) * kPerWave; qw < nq;
         qw += (uint64_t)gridDim.x * kWaves * kPerWave) {
        const uint64_t q = qw + lane / kLceGroup;
        const bool valid = q < nq;
        const uint64_t qc = valid ? q : nq - 1;   // the loads of a query are unconditional: one wait for all of them
        const uint64_t a = qa[qc], b = qb[qc];
        if constexpr (MODE == kLceRanks) {
            uint64_t x = 0, y = 0;
            const bool has = fits && valid && lce_interval_range(a, b, n, x, y);
            const uint32_t m = lce_range_min(lay, lcp, blkw, topw, x, y, has, gl);
            if (valid && gl == 0) static_cast<uint32_t*>(out)[q] = fits && lce_header_ok(h, lay) ? m : kLceNone;
        } else {
            uint32_t ci = 0, cj = 0;
            if constexpr (MODE == kLceOrder) {
                const uint32_t li = la[qc], lj = lb[qc];
                ci = lce_clip(a, li, n);
                cj = lce_clip(b, lj, n);
            }
            const bool both = fits && valid && a < n && b < n;
            const bool two = both && a != b;
            uint32_t ans = both && a == b ? (uint32_t)(n - a) : 0u;
            // the probe: byte gl of both suffixes; past either end counts as the mismatch
            uint32_t ca = 0, cb = 0, mpos = kLceProbe;
            if (text && two) {
                const uint64_t pi = a + gl, pj = b + gl;
                const bool in = pi < n && pj < n;
                if (in) {
                    ca = text[pi];
                    cb = text[pj];
                }
                const uint32_t gm = (uint32_t)(__ballot(!in || ca != cb) >> shift) & 0xFFFFu;
                if (gm) mpos = (uint32_t)__builtin_ctz(gm);
            }
            const bool probed = mpos < kLceProbe;
            const bool need = two && !probed;
            uint32_t va = 0, vb = 0;   // the two ranks: both gathers before either is used
            if (need) {
                va = isa[a];
                vb = isa[b];
            }
            const uint64_t cap = n - 1;   // need: n > 0
            const uint64_t ra = std::min<uint64_t>(va, cap), rb = std::min<uint64_t>(vb, cap);
            const uint64_t x = std::min(ra, rb) + 1, y = std::max(ra, rb);
            const uint32_t m = lce_range_min(lay, lcp, blkw, topw, x, y, need && ra != rb, gl);
            if (probed) ans = mpos;
            if (need) ans = m;
            const bool good = fits && lce_header_ok(h, lay);
            if constexpr (MODE == kLcePositions) {
                if (valid && gl == 0) static_cast<uint32_t*>(out)[q] = good ? ans : kLceNone;
            } else {
                // the bytes at the probe's mismatch (both inside the text when the order needs them)
                const uint32_t src = shift + std::min(mpos, kLceProbe - 1);
                const uint32_t ma = (uint32_t)__shfl((int)ca, (int)src, kWave), mb = (uint32_t)__shfl((int)cb, (int)src, kWave);
                int ord = lce_order(ans, ci, cj);
                if (ord == 2) ord = probed ? (ma < mb ? -1 : 1) : (ra < rb ? -1 : 1);
                if (valid && gl == 0) static_cast<int8_t*>(out)[q] = (int8_t)(good ? ord : 0);
            }
        }
    }
}

// ---- device forms -----------------------------------------------------------
static uint32_t lce_grid(uint64_t items, uint64_t per_group, uint64_t cap) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_group - 1) / per_group, cap));
}

// Host waits: none.  Temporaries: none.  Reads LCP once.
static int lce_build_device(uint64_t n, const uint32_t* d_lcp, void* d_index, uint64_t index_bytes, hipStream_t s) {
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (!d_index) return set_err(SA_E_INVALID, "d_index is NULL");
    if ((uintptr_t)d_index & 15u) return set_err(SA_E_INVALID, "d_index is not 16-byte aligned");
    if (n && !d_lcp) return set_err(SA_E_INVALID, "d_lcp is NULL");
    if ((uintptr_t)d_lcp & 15u) return set_err(SA_E_INVALID, "d_lcp is not 16-byte aligned");
    const LceHeader lay = lce_layout(n);
    if (index_bytes < lay.bytes)
        return set_err(SA_E_INVALID, "index_bytes %llu is below the %llu bytes of the index", (unsigned long long)index_bytes,
                       (unsigned long long)lay.bytes);
    if ((const void*)d_lcp == (const void*)d_index) return set_err(SA_E_INVALID, "d_index may not alias d_lcp");
    uint8_t* base = static_cast<uint8_t*>(d_index);
    uint32_t* blk = reinterpret_cast<uint32_t*>(base + lay.off_blk);
    uint32_t* top = reinterpret_cast<uint32_t*>(base + lay.off_top);
    if (n) {
        hipLaunchKernelGGL(k_lce_blocks, dim3((uint32_t)lay.ns), dim3(kBlock), 0, s, d_lcp, n, lay.nb, blk, top);
        for (uint32_t k = 1; k < lay.levels; ++k)
            hipLaunchKernelGGL(k_lce_top, dim3(lce_grid(lay.ns, kBlock, 1024)), dim3(kBlock), 0, s,
                               (const uint32_t*)(top + (uint64_t)(k - 1) * lay.ns), top + (uint64_t)k * lay.ns, lay.ns,
                               1ull << (k - 1));
    }
    hipLaunchKernelGGL(k_lce_header, dim3(1), dim3(kBlock), 0, s, lay, static_cast<uint32_t*>(d_index));
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// the checks the three query forms share, all before any HIP call; out_align: 4 or 1
static int lce_check_query(uint64_t n, const uint32_t* d_lcp, const void* d_index, uint64_t nq, const void* d_a,
                           const void* d_b, const char* name_a, const char* name_b, const void* d_out,
                           const char* name_out, uint32_t out_align) {
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (!d_index) return set_err(SA_E_INVALID, "d_index is NULL");
    if ((uintptr_t)d_index & 15u) return set_err(SA_E_INVALID, "d_index is not 16-byte aligned");
    if (n && !d_lcp) return set_err(SA_E_INVALID, "d_lcp is NULL");
    if ((uintptr_t)d_lcp & 15u) return set_err(SA_E_INVALID, "d_lcp is not 16-byte aligned");
    if (!d_a) return set_err(SA_E_INVALID, "%s is NULL", name_a);
    if (!d_b) return set_err(SA_E_INVALID, "%s is NULL", name_b);
    if (!d_out) return set_err(SA_E_INVALID, "%s is NULL", name_out);
    if ((uintptr_t)d_out & (out_align - 1u)) return set_err(SA_E_INVALID, "%s is not %u-byte aligned", name_out, out_align);
    if (d_out == d_a || d_out == d_b || d_out == (const void*)d_lcp || d_out == d_index)
        return set_err(SA_E_INVALID, "%s may not alias an input", name_out);
    return SA_OK;
}

// Host waits: none.  Temporaries: none.
static int lcp_min_device(uint64_t n, const uint32_t* d_lcp, const void* d_index, uint64_t index_bytes,
                          const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_out, hipStream_t s) {
    if (nq == 0) return SA_OK;
    SA_TRY(lce_check_query(n, d_lcp, d_index, nq, d_lo, d_hi, "d_lo", "d_hi", d_out, "d_out", 4));
    hipLaunchKernelGGL((k_lce_query<kLceRanks>), dim3(lce_grid(nq, kBlock / kLceGroup, kLceGrid)), dim3(kBlock), 0, s,
                       lce_layout(n), (const uint8_t*)nullptr, (const uint32_t*)nullptr, d_lcp,
                       static_cast<const uint8_t*>(d_index), index_bytes, d_lo, d_hi, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, nq, (void*)d_out);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// Host waits: none.  Temporaries: none.  d_li / d_lj / d_order: the order form (all three or none).
static int lce_positions_device(bool order, uint64_t n, const uint8_t* d_text, const uint32_t* d_isa,
                                const uint32_t* d_lcp, const void* d_index, uint64_t index_bytes, const uint32_t* d_i,
                                const uint32_t* d_j, const uint32_t* d_li, const uint32_t* d_lj, uint64_t nq, void* d_out,
                                hipStream_t s) {
    if (nq == 0) return SA_OK;
    SA_TRY(lce_check_query(n, d_lcp, d_index, nq, d_i, d_j, "d_i", "d_j", d_out, order ? "d_order" : "d_lce",
                           order ? 1 : 4));
    if (n && !d_isa) return set_err(SA_E_INVALID, "d_isa is NULL");
    if (order && !d_li) return set_err(SA_E_INVALID, "d_li is NULL");
    if (order && !d_lj) return set_err(SA_E_INVALID, "d_lj is NULL");
    if (d_out == (const void*)d_isa || d_out == (const void*)d_li || d_out == (const void*)d_lj ||
        (d_text && d_out == (const void*)d_text))
        return set_err(SA_E_INVALID, "%s may not alias an input", order ? "d_order" : "d_lce");
    const dim3 grid(lce_grid(nq, kBlock / kLceGroup, kLceGrid));
    if (order)
        hipLaunchKernelGGL((k_lce_query<kLceOrder>), grid, dim3(kBlock), 0, s, lce_layout(n), d_text, d_isa, d_lcp,
                           static_cast<const uint8_t*>(d_index), index_bytes, d_i, d_j, d_li, d_lj, nq, d_out);
    else
        hipLaunchKernelGGL((k_lce_query<kLcePositions>), grid, dim3(kBlock), 0, s, lce_layout(n), d_text, d_isa, d_lcp,
                           static_cast<const uint8_t*>(d_index), index_bytes, d_i, d_j, (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr, nq, d_out);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// ---- host in, host out, over the steps of sa_host.h ---------------------------
// a width-8 array narrowed to 32 bits (entries outside [0, 2^32 - 1] rejected); *src = the 32-bit entries
static int lce_narrow(const void* a, uint64_t m, int width, const char* what, std::vector<uint32_t>& narrow,
                      const void** src) {
    *src = a;
    if (width == 8) {
        narrow.resize(m);
        const int64_t* w = (const int64_t*)a;
        for (uint64_t i = 0; i < m; ++i) {
            if (w[i] < 0 || (uint64_t)w[i] > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "%s entry out of range", what);
            narrow[i] = (uint32_t)w[i];
        }
        *src = narrow.data();
    }
    return SA_OK;
}

// two uint64 query arrays packed a | b as uint32 for one upload; a value above 2^32 - 1 becomes 2^32 - 1 (>= n)
static void lce_pack(const uint64_t* a, const uint64_t* b, uint64_t nq, uint32_t* dst) {
    for (uint64_t q = 0; q < nq; ++q) {
        dst[q] = (uint32_t)std::min<uint64_t>(a[q], 0xFFFFFFFFull);
        dst[nq + q] = (uint32_t)std::min<uint64_t>(b[q], 0xFFFFFFFFull);
    }
}

static int lcp_min_host(const void* lcp, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                        uint64_t* out) {
    SA_TRY(check_width(width));
    SA_TRY(check_n32(n));
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (nq == 0) return SA_OK;
    if (!lo || !hi) return set_err(SA_E_INVALID, "NULL interval array");
    if (!out) return set_err(SA_E_INVALID, "out is NULL");
    SA_TRY(check_no_alias({out}, {lcp, lo, hi}, "out may not alias an input"));
    if (n && !lcp) return set_err(SA_E_INVALID, "lcp is NULL");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(lce_narrow(lcp, n, width, "LCP", narrow, &src));
    std::vector<uint32_t> lh(2 * nq);
    bool any = false;
    for (uint64_t q = 0; q < nq; ++q) {   // an interval with no minimum stays (0, 0)
        uint64_t x, y;
        const bool has = lce_interval_range(lo[q], hi[q], n, x, y);
        lh[q] = has ? (uint32_t)lo[q] : 0u;
        lh[nq + q] = has ? (uint32_t)hi[q] : 0u;
        any = any || has;
    }
    if (!any) {   // nothing to look up: no device
        std::fill(out, out + nq, (uint64_t)kLceNone);
        return SA_OK;
    }
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    const uint64_t ib = lce_index_bytes(n);
    DevBuf d_lcp, d_idx, d_lh, d_out;
    SA_TRY(d_lcp.alloc(align_up(n, 64) * 4));
    SA_TRY(d_idx.alloc(ib));
    SA_TRY(d_lh.alloc(align_up(2 * nq, 64) * 4));
    SA_TRY(d_out.alloc(align_up(nq, 64) * 4));
    SA_TRY(upload({{d_lcp.p, src, n * 4}, {d_lh.p, lh.data(), 2 * nq * 4}}));
    SA_TRY(lce_build_device(n, d_lcp.as<uint32_t>(), d_idx.p, ib, nullptr));
    SA_TRY(lcp_min_device(n, d_lcp.as<uint32_t>(), d_idx.p, ib, d_lh.as<uint32_t>(), d_lh.as<uint32_t>() + nq, nq,
                          d_out.as<uint32_t>(), nullptr));
    return download_u64({{out, d_out.as<uint32_t>()}}, nq);
}

// sa_lce (li == NULL) and sa_substr_compare: LCP, ISA and the index are computed here, the text is probed
static int lce_positions_host(bool order, const uint8_t* text, uint64_t n, const void* sa, int sa_width,
                              const uint64_t* i, const uint64_t* li, const uint64_t* j, const uint64_t* lj, uint64_t nq,
                              void* out) {
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (nq == 0) return SA_OK;
    if (!i || !j) return set_err(SA_E_INVALID, "NULL position array");
    if (order && (!li || !lj)) return set_err(SA_E_INVALID, "NULL length array");
    if (!out) return set_err(SA_E_INVALID, "out is NULL");
    SA_TRY(check_no_alias({out}, {i, j, li, lj, text, sa}, "out may not alias an input"));
    if (n && (!text || !sa)) return set_err(SA_E_INVALID, "NULL host pointer");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    if (n == 0) {   // every position is the empty suffix
        if (order) std::memset(out, 0, nq);
        else std::fill((uint64_t*)out, (uint64_t*)out + nq, 0ull);
        return SA_OK;
    }
    std::vector<uint32_t> qs((order ? 4 : 2) * nq);
    lce_pack(i, j, nq, qs.data());
    if (order) lce_pack(li, lj, nq, qs.data() + 2 * nq);
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    const uint64_t ib = lce_index_bytes(n);
    DevBuf d_text, d_sa, d_lcp, d_isa, d_idx, d_q, d_out;
    SA_TRY(d_text.alloc(align_up(n, 256)));
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_lcp.alloc(align_up(n, 64) * 4));
    SA_TRY(d_isa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_idx.alloc(ib));
    SA_TRY(d_q.alloc(align_up(qs.size(), 64) * 4));
    SA_TRY(d_out.alloc(align_up(nq, 64) * 4));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}, {d_q.p, qs.data(), qs.size() * 4}}));
    // the checker rejects a non-permutation before PHI would scatter through it
    const int ok = check_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), nullptr);
    if (ok == 0) return set_err(SA_E_INVALID, "not a valid suffix array of the text");
    if (ok != 1) return ok;
    SA_TRY(lcp_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_lcp.as<uint32_t>(), nullptr, nullptr));
    SA_TRY(inverse_device(c, n, d_sa.as<uint32_t>(), d_isa.as<uint32_t>(), nullptr));
    SA_TRY(lce_build_device(n, d_lcp.as<uint32_t>(), d_idx.p, ib, nullptr));
    const uint32_t* dq = d_q.as<uint32_t>();
    SA_TRY(lce_positions_device(order, n, d_text.as<uint8_t>(), d_isa.as<uint32_t>(), d_lcp.as<uint32_t>(), d_idx.p, ib, dq,
                                dq + nq, order ? dq + 2 * nq : nullptr, order ? dq + 3 * nq : nullptr, nq, d_out.p,
                                nullptr));
    if (!order) return download_u64({{(uint64_t*)out, d_out.as<uint32_t>()}}, nq);
    SA_HIP(hipMemcpyAsync(out, d_out.p, nq, hipMemcpyDeviceToHost, nullptr));
    SA_HIP(host_sync(nullptr));
    return SA_OK;
}

}  // namespace sa

extern "C" {

uint64_t sa_lce_index_bytes(uint64_t n) { return n > 0xFFFFFFFFull ? 0 : sa::lce_index_bytes(n); }

int sa_lce_build_device(uint64_t n, const uint32_t* d_lcp, void* d_index, uint64_t index_bytes, void* stream) {
    return sa::lce_build_device(n, d_lcp, d_index, index_bytes, (hipStream_t)stream);
}

int sa_lcp_min_device(uint64_t n, const uint32_t* d_lcp, const void* d_index, uint64_t index_bytes, const uint32_t* d_lo,
                      const uint32_t* d_hi, uint64_t nq, uint32_t* d_out, void* stream) {
    return sa::lcp_min_device(n, d_lcp, d_index, index_bytes, d_lo, d_hi, nq, d_out, (hipStream_t)stream);
}

int sa_lce_device(uint64_t n, const uint8_t* d_text, const uint32_t* d_isa, const uint32_t* d_lcp, const void* d_index,
                  uint64_t index_bytes, const uint32_t* d_i, const uint32_t* d_j, uint64_t nq, uint32_t* d_lce,
                  void* stream) {
    return sa::lce_positions_device(false, n, d_text, d_isa, d_lcp, d_index, index_bytes, d_i, d_j, nullptr, nullptr, nq,
                                    d_lce, (hipStream_t)stream);
}

int sa_substr_compare_device(uint64_t n, const uint8_t* d_text, const uint32_t* d_isa, const uint32_t* d_lcp,
                             const void* d_index, uint64_t index_bytes, const uint32_t* d_i, const uint32_t* d_li,
                             const uint32_t* d_j, const uint32_t* d_lj, uint64_t nq, int8_t* d_order, void* stream) {
    return sa::lce_positions_device(true, n, d_text, d_isa, d_lcp, d_index, index_bytes, d_i, d_j, d_li, d_lj, nq, d_order,
                                    (hipStream_t)stream);
}

int sa_lcp_min(const void* lcp, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
               uint64_t* out) {
    return sa::lcp_min_host(lcp, n, width, lo, hi, nq, out);
}

int sa_lce(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint64_t* i, const uint64_t* j,
           uint64_t nq, uint64_t* out) {
    return sa::lce_positions_host(false, text, n, sa, sa_width, i, nullptr, j, nullptr, nq, out);
}

int sa_substr_compare(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint64_t* i,
                      const uint64_t* li, const uint64_t* j, const uint64_t* lj, uint64_t nq, int8_t* out) {
    return sa::lce_positions_host(true, text, n, sa, sa_width, i, li, j, lj, nq, out);
}

}  // extern "C"

#endif   // __HIPCC__
