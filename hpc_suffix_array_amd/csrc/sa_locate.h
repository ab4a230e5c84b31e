// sa_locate.h -- batched locate: the text positions of nq SA intervals as
// sorted hit lists in CSR form (sa_locate / sa_locate_device of
// include/sa_hip.h).
//
// c[q] = min(hi[q] - lo[q], max_hits or infinity), 0 for an interval that
// breaks lo <= hi <= n; off = the exclusive sum of c (nq + 1 uint64); pos[off[q]
// .. off[q + 1]) = SA[lo[q] .. lo[q] + c[q]), ascending (or as they lie in the
// SA with SA_LOCATE_SA_ORDER).  The text is never read.
//
//   k_locate_count   c[q] into off[q + 1], the large queries (c > kLocateTile)
//                    and their hits counted into two words; off is then summed
//                    in place by scan_i64<ScanSum>.
//   k_locate_small   the hot path.  The output is cut into tiles of
//                    kLocateTile slots; a query belongs to the tile that holds
//                    its first hit, so a workgroup holds fewer than
//                    2 * kLocateTile hits (locate_tile below).  The workgroup
//                    marks its queries' first slots in LDS, spreads them over
//                    the slots by a max-scan, gathers SA[lo[q] + (slot - first
//                    slot)] with consecutive lanes on consecutive slots (coalesced
//                    inside an interval), and sorts the whole tile once in LDS by
//                    the composite key (first slot of the query, position): the
//                    slots are already grouped by query, so one sort orders every
//                    segment.  When no segment of the tile is longer than
//                    kLocRankMax the sort is a rank by counting inside the segment
//                    (at most kLocRankMax LDS reads per hit, two barriers);
//                    otherwise a bitonic network over the next power of two.  The
//                    grid is persistent and reads the total on the device, so
//                    the kernel is launched before the host knows the total.
//                    A large query is the last one that starts in its tile and
//                    is left out of it.
//   large class      after the one host wait: k_locate_list compacts the large
//                    queries, k_locate_expand writes composite keys (index among
//                    the large queries, position) with the position as value,
//                    the context's LSD radix sort (sa_sort_pairs_device) orders
//                    them over bits(n) + bits(n_large) key bits and
//                    k_locate_narrow copies each query's sorted values to its
//                    place in d_pos, 16 bytes per store inside locate_split's
//                    body.  More than kLocateSortMax large hits are sorted in
//                    several chunks cut between queries.
//
// The arithmetic (capped count and class, a tile's queries, the composite key,
// the split of an output range for 16-byte stores) compiles on the host:
// tests/cpp/locate_check.cpp checks it against brute force.
// Measurements and the resource report: DESIGN.md section 13.
// The HIP part needs sa_host.h before it (the host form's staging, buffers,
// checks and the process-wide context), and sa_build.hip's scan_i64 and
// sa_sort_pairs_device.
#pragma once
#include <stdint.h>

#include "sa_search.h"   // SA_HD

namespace sa {

// output slots per tile, and the largest query of the small class
// (= SA_LOCATE_TILE = _native.LOCATE_TILE)
constexpr uint32_t kLocateTile = 2048;

// hits of query [lo, hi) under the cap (0 = none); an interval that breaks
// lo <= hi <= n is empty.  n <= 2^32 - 1, so the count fits 32 bits.
SA_HD uint32_t locate_count(uint64_t lo, uint64_t hi, uint64_t n, uint64_t max_hits) {
    if (lo > hi || hi > n) return 0u;
    uint64_t c = hi - lo;
    if (max_hits && c > max_hits) c = max_hits;
    return (uint32_t)c;
}

// the class is decided on the capped count
SA_HD bool locate_large(uint64_t c) { return c > kLocateTile; }

// first i in [a, b) with off(i) >= x, else b (off non-decreasing)
template <class Off>
SA_HD uint64_t locate_lower_bound(const Off& off, uint64_t a, uint64_t b, uint64_t x) {
    uint64_t len = b - a;
    while (len > 0) {
        const uint64_t half = len >> 1;
        if (off(a + half) < x) {
            a += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return a;
}

// first query of tile t: the first q with off(q) >= t * kLocateTile (nq when
// there is none).  It may be an empty query in front of the tile's first hit.
template <class Off>
SA_HD uint64_t locate_tile_first(const Off& off, uint64_t nq, uint64_t t) {
    return locate_lower_bound(off, 0, nq, t * kLocateTile);
}

// The small queries of tile t: queries [q0, q1), output slots [s, e), with
// e - s < 2 * kLocateTile.  off has nq + 1 entries.  The queries that start in
// the tile end where the next tile's first query starts; if the last non-empty
// one of them is large (only the last can be: it covers the rest of the tile)
// the range ends in front of it.
struct LocateTile {
    uint64_t q0, q1, s, e;
};
template <class Off>
SA_HD LocateTile locate_tile(const Off& off, uint64_t nq, uint64_t t) {
    LocateTile r;
    r.q0 = locate_tile_first(off, nq, t);
    r.q1 = locate_lower_bound(off, r.q0, nq, (t + 1) * kLocateTile);
    r.s = off(r.q0);
    r.e = off(r.q1);
    if (r.e > r.s) {
        // the last non-empty query is the one before the first index that reaches e
        const uint64_t last = locate_lower_bound(off, r.q0, r.q1, r.e) - 1;
        if (locate_large(r.e - off(last))) {
            r.q1 = last;
            r.e = off(last);
        }
    }
    return r;
}

// bits that hold every value of [0, x): 0 for x <= 1
SA_HD uint32_t locate_bits(uint64_t x) {
    uint32_t b = 0;
    if (x > 1)
        while (b < 64 && ((x - 1) >> b)) ++b;
    return b;
}
// composite key of the large class: (index among the chunk's large queries,
// position), positions in bits(n) bits
SA_HD uint32_t locate_key_bits(uint64_t n, uint64_t n_large) { return locate_bits(n) + locate_bits(n_large); }
SA_HD uint64_t locate_key(uint64_t j, uint32_t pos, uint32_t pos_bits) {
    const uint64_t mask = (1ull << pos_bits) - 1ull;   // pos_bits <= 32
    return (j << pos_bits) | ((uint64_t)pos & mask);
}
SA_HD uint64_t locate_key_query(uint64_t key, uint32_t pos_bits) { return key >> pos_bits; }
SA_HD uint32_t locate_key_pos(uint64_t key, uint32_t pos_bits) {
    return (uint32_t)(key & ((1ull << pos_bits) - 1ull));
}

// An output range of `total` 4-byte entries that starts `first` entries past
// a 16-byte boundary (first = (address / 4) % 4): `head` entries up to the
// boundary and `tail` entries after the last whole group are stored one by
// one, the `body` (a multiple of 4) as 16-byte groups.
struct LocateSplit {
    uint32_t head;
    uint64_t body;
    uint32_t tail;
};
SA_HD LocateSplit locate_split(uint32_t first, uint64_t total) {
    LocateSplit r;
    const uint64_t h = (4u - (first & 3u)) & 3u;
    r.head = (uint32_t)(h < total ? h : total);
    r.body = (total - r.head) & ~3ull;
    r.tail = (uint32_t)(total - r.head - r.body);
    return r;
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

#include "sa_kernels.h"

namespace sa {

static_assert(kLocateTile == SA_LOCATE_TILE, "the header's tile constant");
constexpr uint32_t kLocSlots = 2 * kLocateTile;          // LDS slots of a workgroup (> its hits)
constexpr int kLocPer = (int)(kLocSlots / kBlock);       // slots per lane
constexpr uint32_t kLocRankMax = 64;                     // longest segment ranked by counting
constexpr uint32_t kLocGridPerCu = 4;                    // workgroups per CU of the persistent grid
constexpr uint64_t kLocateSortMax = 1ull << 28;          // large hits sorted in one call
constexpr uint64_t kLocateTestChunk = 1ull << 14;        // SA_LOCATE_SMALL_CHUNKS
static_assert(kLocPer == 16 && kLocSlots <= 65536, "16 slots per lane, 16-bit slot numbers");

typedef uint32_t loc_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

struct LocOff {
    const uint64_t* __restrict__ p;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return p[i]; }
};
// ends of the listed large queries: entry j is ls[j + 1]
struct LocEnds {
    const int64_t* __restrict__ p;
    __device__ __forceinline__ uint64_t operator()(uint64_t j) const { return (uint64_t)p[j + 1]; }
};

__global__ __launch_bounds__(kBlock) void k_locate_count(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                         uint64_t nq, uint64_t n, uint64_t max_hits,
                                                         uint64_t* __restrict__ off,
                                                         unsigned long long* __restrict__ words) {
    unsigned long long nl = 0, lh = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = locate_count(lo[q], hi[q], n, max_hits);
        off[q + 1] = c;
        if (locate_large(c)) {
            ++nl;
            lh += c;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[0] = 0;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        nl += __shfl_down(nl, o, kWave);
        lh += __shfl_down(lh, o, kWave);
    }
    if (lane_id() == 0 && nl) {
        atomicAdd(&words[0], nl);
        atomicAdd(&words[1], lh);
    }
}

template <bool SORT>
__global__ __launch_bounds__(kBlock) void k_locate_small(const uint32_t* __restrict__ sa, uint64_t n,
                                                         const uint32_t* __restrict__ lo, uint64_t nq,
                                                         const uint64_t* __restrict__ off, uint32_t* __restrict__ pos,
                                                         uint64_t pos_cap) {
    // the sort's keys; before them the same bytes hold, per slot, the query
    // that starts there (s_q, + 1, 0 none) and the first slot of the slot's
    // query (s_seg)
    __shared__ __attribute__((aligned(16))) uint64_t s_key[kLocSlots];
    __shared__ uint32_t s_wmax[kWaves];
    __shared__ uint32_t s_maxlen;
    uint32_t* s_q = reinterpret_cast<uint32_t*>(s_key);
    uint16_t* s_seg = reinterpret_cast<uint16_t*>(s_q + kLocSlots);
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = lane_id(), wave = tid / kWave;
    const uint64_t total = off[nq];
    if (total > pos_cap) return;   // the sizing case: the host sees the same total
    const uint64_t tiles = (total + kLocateTile - 1) / kLocateTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const LocateTile r = locate_tile(LocOff{off}, nq, t);
        const uint32_t cnt = (uint32_t)(r.e - r.s);   // < kLocSlots
        if (cnt == 0 || cnt >= kLocSlots) continue;   // uniform; the second never holds for a summed off
        for (uint32_t i = tid; i < kLocSlots; i += kBlock) s_q[i] = 0u;
        if (tid == 0) s_maxlen = 0u;
        __syncthreads();
        uint32_t ml = 0;
        for (uint64_t q = r.q0 + tid; q < r.q1; q += kBlock) {
            const uint64_t a = off[q], b = off[q + 1];
            if (b > a && a >= r.s && b <= r.e) {
                s_q[a - r.s] = (uint32_t)(q - r.q0) + 1u;
                ml = std::max(ml, (uint32_t)(b - a));
            }
        }
        if (SORT && ml > kLocRankMax) atomicMax(&s_maxlen, ml);
        __syncthreads();
        // first slot of each slot's query: the last marked slot at or below
        // it, a max-scan over the lanes' 16 contiguous slots
        {
            const uint4* mine = reinterpret_cast<const uint4*>(s_q + kLocPer * tid);
            uint32_t m[kLocPer];
#pragma unroll
            for (int j = 0; j < kLocPer / 4; ++j) {
                const uint4 v = mine[j];
                m[4 * j] = v.x;
                m[4 * j + 1] = v.y;
                m[4 * j + 2] = v.z;
                m[4 * j + 3] = v.w;
            }
            uint32_t last = 0;   // slot + 1 of the lane's last marked slot
#pragma unroll
            for (int j = 0; j < kLocPer; ++j)
                if (m[j]) last = kLocPer * tid + j + 1u;
            uint32_t incl = last;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o, kWave);
                if ((int)lane >= o) incl = std::max(incl, y);
            }
            if (lane == kWave - 1) s_wmax[wave] = incl;
            __syncthreads();
            uint32_t cur = (uint32_t)__shfl_up((int)incl, 1, kWave);
            if (lane == 0) cur = 0u;
            for (uint32_t w = 0; w < wave; ++w) cur = std::max(cur, s_wmax[w]);
            uint32_t seg[kLocPer];
#pragma unroll
            for (int j = 0; j < kLocPer; ++j) {
                if (m[j]) cur = kLocPer * tid + j + 1u;
                seg[j] = cur ? cur - 1u : 0u;   // slot 0 is marked: cur > 0 for every used slot
            }
            uint4* out = reinterpret_cast<uint4*>(s_seg + kLocPer * tid);
#pragma unroll
            for (int j = 0; j < kLocPer / 8; ++j)
                out[j] = make_uint4(seg[8 * j] | (seg[8 * j + 1] << 16), seg[8 * j + 2] | (seg[8 * j + 3] << 16),
                                    seg[8 * j + 4] | (seg[8 * j + 5] << 16), seg[8 * j + 6] | (seg[8 * j + 7] << 16));
        }
        __syncthreads();
        // gather: lane l of pass j has slot j * 256 + l
        uint64_t key[kLocPer];
#pragma unroll
        for (int j = 0; j < kLocPer; ++j) {
            const uint32_t i = j * kBlock + tid;
            key[j] = ~0ull;
            const uint32_t s = i < cnt ? s_seg[i] : 0u;
            const uint32_t qi = s_q[s] - 1u;
            if (i < cnt && qi < r.q1 - r.q0) {   // the second holds: slot s is marked
                const uint64_t at = std::min<uint64_t>((uint64_t)lo[r.q0 + qi] + (i - s), n - 1);
                const uint32_t p = sa[at];
                if constexpr (SORT) key[j] = ((uint64_t)s << 32) | p;
                else pos[r.s + i] = p;
            }
        }
        __syncthreads();   // s_q and s_seg are read: the keys may take their place
        if constexpr (SORT) {
            if (s_maxlen == 0u) {
                // short segments: rank inside the segment.  The slot after
                // the last hit holds a key of no segment and ends the scan.
#pragma unroll
                for (int j = 0; j < kLocPer; ++j) {
                    const uint32_t i = j * kBlock + tid;
                    if (i <= cnt) s_key[i] = key[j];
                }
                __syncthreads();
                uint32_t dst[kLocPer];
#pragma unroll
                for (int j = 0; j < kLocPer; ++j) {
                    const uint32_t i = j * kBlock + tid;
                    dst[j] = i;
                    if (i < cnt) {
                        const uint32_t s = (uint32_t)(key[j] >> 32);
                        uint32_t rank = 0;
                        for (uint32_t k = s; k < kLocSlots; ++k) {
                            const uint64_t x = s_key[k];
                            if ((uint32_t)(x >> 32) != s) break;
                            rank += (x < key[j] || (x == key[j] && k < i)) ? 1u : 0u;
                        }
                        dst[j] = s + rank;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kLocPer; ++j)
                    if (j * kBlock + tid < cnt) s_key[dst[j]] = key[j];
            } else {
                uint32_t P = 2 * kBlock;
                while (P < cnt) P <<= 1;   // <= kLocSlots
#pragma unroll
                for (int j = 0; j < kLocPer; ++j) s_key[j * kBlock + tid] = key[j];
                __syncthreads();
                for (uint32_t k = 2; k <= P; k <<= 1) {
                    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                        for (uint32_t p = tid; p < P / 2; p += kBlock) {
                            const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));
                            const uint32_t l = i | j;
                            const uint64_t a = s_key[i], b = s_key[l];
                            if ((a > b) == ((i & k) == 0u)) {
                                s_key[i] = b;
                                s_key[l] = a;
                            }
                        }
                        __syncthreads();
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kLocPer; ++j) {
                const uint32_t i = j * kBlock + tid;
                if (i < cnt) pos[r.s + i] = (uint32_t)s_key[i];
            }
            __syncthreads();   // the next tile clears these bytes
        }
    }
}

// the large queries in some order: lq[j] = q, ls[j + 1] = c[q] (summed after)
__global__ __launch_bounds__(kBlock) void k_locate_list(const uint64_t* __restrict__ off, uint64_t nq,
                                                        unsigned long long* __restrict__ counter,
                                                        uint64_t* __restrict__ lq, int64_t* __restrict__ ls,
                                                        uint64_t n_large) {
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock) {
        const uint64_t c = off[q + 1] - off[q];
        if (locate_large(c)) {
            const unsigned long long j = atomicAdd(counter, 1ull);
            if (j < n_large) {
                lq[j] = q;
                ls[j + 1] = (int64_t)c;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ls[0] = 0;
}

// hits [e0, e0 + m) of the listed large queries [j0, j1): key (j - j0,
// position), value the position; DIRECT (SA order, nothing to sort): the
// position straight to its place in pos (keys = the offsets, vals = pos)
template <bool DIRECT>
__global__ __launch_bounds__(kBlock) void k_locate_expand(const uint32_t* __restrict__ sa, uint64_t n,
                                                          const uint32_t* __restrict__ lo,
                                                          const uint64_t* __restrict__ lq,
                                                          const int64_t* __restrict__ ls, uint64_t j0, uint64_t j1,
                                                          uint64_t e0, uint64_t m, uint32_t pos_bits,
                                                          uint64_t* keys, uint32_t* vals) {
    for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < m; x += (uint64_t)gridDim.x * kBlock) {
        const uint64_t e = e0 + x;
        const uint64_t j = std::min<uint64_t>(locate_lower_bound(LocEnds{ls}, j0, j1, e + 1), j1 - 1);
        const uint64_t at = std::min<uint64_t>((uint64_t)lo[lq[j]] + (e - (uint64_t)ls[j]), n - 1);
        const uint32_t p = sa[at];
        if constexpr (DIRECT) {
            vals[keys[lq[j]] + (e - (uint64_t)ls[j])] = p;
        } else {
            keys[x] = locate_key(j - j0, p, pos_bits);
            vals[x] = p;
        }
    }
}

// sorted values of the listed large queries [j0, j1) (from hit e0 on) to
// their places in pos; blockIdx.y shares a query's 16-byte groups
__global__ __launch_bounds__(kBlock) void k_locate_narrow(const uint32_t* __restrict__ sorted,
                                                          const uint64_t* __restrict__ lq,
                                                          const int64_t* __restrict__ ls, uint64_t j0, uint64_t j1,
                                                          uint64_t e0, const uint64_t* __restrict__ off,
                                                          uint32_t* __restrict__ pos) {
    const uint32_t tid = threadIdx.x;
    for (uint64_t j = j0 + blockIdx.x; j < j1; j += gridDim.x) {
        const uint32_t* __restrict__ src = sorted + ((uint64_t)ls[j] - e0);
        const uint64_t c = (uint64_t)(ls[j + 1] - ls[j]);
        uint32_t* __restrict__ dst = pos + off[lq[j]];
        const LocateSplit sp = locate_split((uint32_t)(((uintptr_t)dst >> 2) & 3u), c);
        if (blockIdx.y == 0) {
            if (tid < sp.head) dst[tid] = src[tid];
            if (tid < sp.tail) dst[sp.head + sp.body + tid] = src[sp.head + sp.body + tid];
        }
        const uint64_t groups = sp.body >> 2;
        for (uint64_t g = (uint64_t)blockIdx.y * kBlock + tid; g < groups; g += (uint64_t)gridDim.y * kBlock) {
            const loc_u32x4 v = *reinterpret_cast<const loc_u32x4*>(src + sp.head + 4 * g);
            *reinterpret_cast<uint4*>(dst + sp.head + 4 * g) = make_uint4(v.x, v.y, v.z, v.w);
        }
    }
}

// a stream-ordered allocation freed on every path
struct LocBuf {
    void* p = nullptr;
    hipStream_t s = nullptr;
    int alloc(size_t bytes, hipStream_t stream) {
        s = stream;
        if (hipMallocAsync(&p, bytes, s) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return set_err(SA_E_NOMEM, "device allocation of %zu bytes failed", bytes);
        }
        return SA_OK;
    }
    ~LocBuf() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

// the empty answer in CSR form: rows + 1 zero offsets, waited for
static int empty_csr(uint64_t* d_off, uint64_t rows, hipStream_t s) {
    SA_HIP(hipMemsetAsync(d_off, 0, (rows + 1) * 8, s));
    SA_HIP(host_sync(s));
    return SA_OK;
}

// the checks of sa_locate_device, all before any HIP call
static int locate_check_args(const sa_context* c, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lo,
                             const uint32_t* d_hi, uint64_t nq, uint32_t flags, const uint64_t* d_off,
                             const uint32_t* d_pos, const uint64_t* total) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!total) return set_err(SA_E_INVALID, "total is NULL");
    if (!d_sa) return set_err(SA_E_INVALID, "d_sa is NULL");
    if (!d_lo) return set_err(SA_E_INVALID, "d_lo is NULL");
    if (!d_hi) return set_err(SA_E_INVALID, "d_hi is NULL");
    if (!d_off) return set_err(SA_E_INVALID, "d_off is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (d_pos && (const void*)d_pos == (const void*)d_sa) return set_err(SA_E_INVALID, "d_pos may not alias d_sa");
    return check_flags(flags, SA_LOCATE_SA_ORDER | SA_LOCATE_SMALL_CHUNKS);
}

// Host waits: one when no query is large (or nothing is written); with large
// queries one more per sorted chunk (the radix sort's own), one when the
// chunks have to be cut on the host, and one at the end.
// pos_n: the entries of d_sa are below pos_n (n for a suffix array; sa_fm.h
// sorts hit lists whose entries are text positions of a longer text)
static int locate_device_n(sa_context* c, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lo, const uint32_t* d_hi,
                           uint64_t nq, uint64_t max_hits, uint32_t flags, uint64_t* d_off, uint32_t* d_pos,
                           uint64_t pos_cap, uint64_t* total, hipStream_t s, uint64_t pos_n) {
    SA_TRY(locate_check_args(c, n, d_sa, d_lo, d_hi, nq, flags, d_off, d_pos, total));
    *total = 0;
    SA_HIP(hipSetDevice(c->device));
    if (nq == 0) return empty_csr(d_off, 0, s);
    uint64_t* h = host_u64<kHwLocate, 3>(c);
    {
        LocBuf w;
        SA_TRY(w.alloc(16, s));
        SA_HIP(hipMemsetAsync(w.p, 0, 16, s));
        const uint32_t grid =
            (uint32_t)std::min<uint64_t>((nq + kBlock - 1) / kBlock, (uint64_t)c->cus * 8);
        hipLaunchKernelGGL(k_locate_count, dim3(grid), dim3(kBlock), 0, s, d_lo, d_hi, nq, n, max_hits, d_off,
                           (unsigned long long*)w.p);
        SA_HIP(hipGetLastError());
        SA_TRY(scan_i64<ScanSum>(reinterpret_cast<int64_t*>(d_off) + 1, nq, s));
        if (d_pos) {
            // tiles <= nq * (the largest count) / kLocateTile + 1; the grid is capped and strides
            const uint64_t per = std::min<uint64_t>(max_hits ? max_hits : n, n);
            const uint64_t bound = per ? (nq * per + kLocateTile - 1) / kLocateTile : 1;   // < 2^64: both < 2^32
            const uint32_t g = (uint32_t)std::max<uint64_t>(
                1, std::min<uint64_t>(bound, (uint64_t)c->cus * kLocGridPerCu));
            if (flags & SA_LOCATE_SA_ORDER)
                hipLaunchKernelGGL((k_locate_small<false>), dim3(g), dim3(kBlock), 0, s, d_sa, n, d_lo, nq,
                                   (const uint64_t*)d_off, d_pos, pos_cap);
            else
                hipLaunchKernelGGL((k_locate_small<true>), dim3(g), dim3(kBlock), 0, s, d_sa, n, d_lo, nq,
                                   (const uint64_t*)d_off, d_pos, pos_cap);
            SA_HIP(hipGetLastError());
        }
        SA_HIP(hipMemcpyAsync(h, d_off + nq, 8, hipMemcpyDeviceToHost, s));
        SA_HIP(hipMemcpyAsync(h + 1, w.p, 16, hipMemcpyDeviceToHost, s));
    }
    SA_HIP(host_sync(s));
    *total = h[0];
    const uint64_t n_large = h[1], large_hits = h[2];
    SA_TRACE("locate: nq %llu total %llu large %llu (%llu hits)", (unsigned long long)nq, (unsigned long long)h[0],
             (unsigned long long)n_large, (unsigned long long)large_hits);
    if (!d_pos || *total > pos_cap || n_large == 0) return SA_OK;

    // ---- large class ----
    LocBuf list;   // counter (16 bytes) | ls (n_large + 1) | lq (n_large)
    SA_TRY(list.alloc(16 + (2 * n_large + 1) * 8, s));
    unsigned long long* d_counter = (unsigned long long*)list.p;
    int64_t* d_ls = (int64_t*)list.p + 2;
    uint64_t* d_lq = (uint64_t*)(d_ls + n_large + 1);
    SA_HIP(hipMemsetAsync(list.p, 0, 16 + (2 * n_large + 1) * 8, s));   // an unlisted entry is query 0, no hits
    {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nq + kBlock - 1) / kBlock, (uint64_t)c->cus * 8);
        hipLaunchKernelGGL(k_locate_list, dim3(grid), dim3(kBlock), 0, s, (const uint64_t*)d_off, nq, d_counter, d_lq,
                           d_ls, n_large);
        SA_HIP(hipGetLastError());
    }
    SA_TRY(scan_i64<ScanSum>(d_ls + 1, n_large, s));
    if (flags & SA_LOCATE_SA_ORDER) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((large_hits + kBlock - 1) / kBlock, (uint64_t)c->cus * 16);
        hipLaunchKernelGGL((k_locate_expand<true>), dim3(grid), dim3(kBlock), 0, s, d_sa, n, d_lo,
                           (const uint64_t*)d_lq, (const int64_t*)d_ls, (uint64_t)0, n_large, (uint64_t)0, large_hits,
                           0u, d_off, d_pos);
        SA_HIP(hipGetLastError());
        SA_HIP(host_sync(s));
        return SA_OK;
    }
    // chunks of whole queries, each sorted by one call: cuts[i] = (first query, first hit)
    const uint64_t chunk_max = (flags & SA_LOCATE_SMALL_CHUNKS) ? kLocateTestChunk : kLocateSortMax;
    std::vector<std::pair<uint64_t, uint64_t>> cuts;
    cuts.emplace_back(0, 0);
    if (large_hits > chunk_max) {
        std::vector<int64_t> h_ls(n_large + 1);
        SA_HIP(hipMemcpyAsync(h_ls.data(), d_ls, (n_large + 1) * 8, hipMemcpyDeviceToHost, s));
        SA_HIP(host_sync(s));
        for (uint64_t j = 1; j < n_large; ++j)
            if ((uint64_t)h_ls[j + 1] - cuts.back().second > chunk_max && j > cuts.back().first)
                cuts.emplace_back(j, (uint64_t)h_ls[j]);
    }
    cuts.emplace_back(n_large, large_hits);
    const uint32_t pos_bits = locate_bits(pos_n);
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const uint64_t j0 = cuts[k].first, j1 = cuts[k + 1].first;
        const uint64_t e0 = cuts[k].second, m = cuts[k + 1].second - e0;
        if (m == 0 || m > 0xFFFFFFFFull) return set_err(SA_E_INTERNAL, "locate: a chunk of %llu large hits",
                                                        (unsigned long long)m);
        LocBuf tmp;   // keys in | keys out | values in | values out
        SA_TRY(tmp.alloc(m * 24, s));
        uint64_t* k_in = (uint64_t*)tmp.p;
        uint64_t* k_out = k_in + m;
        uint32_t* v_in = (uint32_t*)(k_out + m);
        uint32_t* v_out = v_in + m;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((m + kBlock - 1) / kBlock, (uint64_t)c->cus * 16);
        hipLaunchKernelGGL((k_locate_expand<false>), dim3(grid), dim3(kBlock), 0, s, d_sa, n, d_lo, (const uint64_t*)d_lq,
                           (const int64_t*)d_ls, j0, j1, e0, m, pos_bits, k_in, v_in);
        SA_HIP(hipGetLastError());
        SA_TRY(sa_sort_pairs_device(c, k_in, v_in, m, pos_bits + locate_bits(j1 - j0), k_out, v_out, s));
        hipLaunchKernelGGL(k_locate_narrow, dim3((uint32_t)std::min<uint64_t>(j1 - j0, 1024), 32), dim3(kBlock), 0, s,
                           (const uint32_t*)v_out, (const uint64_t*)d_lq, (const int64_t*)d_ls, j0, j1, e0,
                           (const uint64_t*)d_off, d_pos);
        SA_HIP(hipGetLastError());
    }
    SA_HIP(host_sync(s));
    return SA_OK;
}

static int locate_device(sa_context* c, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lo, const uint32_t* d_hi,
                         uint64_t nq, uint64_t max_hits, uint32_t flags, uint64_t* d_off, uint32_t* d_pos,
                         uint64_t pos_cap, uint64_t* total, hipStream_t s) {
    return locate_device_n(c, n, d_sa, d_lo, d_hi, nq, max_hits, flags, d_off, d_pos, pos_cap, total, s, n);
}

// the host forms' intervals checked against [0, n] and packed lo | hi for one upload;
// off_out (when given, off_out[0] = 0) takes the sums of their hits under max_hits
static int pack_intervals(const uint64_t* lo, const uint64_t* hi, uint64_t nq, uint64_t n, uint64_t max_hits,
                          uint64_t* off_out, std::vector<uint32_t>& lh) {
    if (!lo || !hi) return set_err(SA_E_INVALID, "NULL interval array");
    lh.resize(2 * nq);
    for (uint64_t q = 0; q < nq; ++q) {
        if (lo[q] > hi[q] || hi[q] > n)
            return set_err(SA_E_INVALID, "interval %llu is [%llu, %llu) of %llu", (unsigned long long)q,
                           (unsigned long long)lo[q], (unsigned long long)hi[q], (unsigned long long)n);
        if (off_out) off_out[q + 1] = off_out[q] + locate_count(lo[q], hi[q], n, max_hits);
        lh[q] = (uint32_t)lo[q];
        lh[nq + q] = (uint32_t)hi[q];
    }
    return SA_OK;
}

// host in, host out (sa_locate), over the steps of sa_host.h: the offsets and
// the total are the host's own
static int locate_host(const void* sa, uint64_t n, int sa_width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                       uint64_t max_hits, uint32_t flags, uint64_t* off_out, void* pos_out, uint64_t pos_cap) {
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    SA_TRY(check_flags(flags, SA_LOCATE_SA_ORDER | SA_LOCATE_SMALL_CHUNKS));
    if (!off_out) return set_err(SA_E_INVALID, "off_out is NULL");
    off_out[0] = 0;
    if (nq == 0) return SA_OK;
    std::vector<uint32_t> lh;
    SA_TRY(pack_intervals(lo, hi, nq, n, max_hits, off_out, lh));
    const uint64_t total = off_out[nq];
    if (pos_cap < total)
        return set_err(SA_E_INVALID, "pos_cap %llu is below the %llu hits", (unsigned long long)pos_cap,
                       (unsigned long long)total);
    if (n && !sa) return set_err(SA_E_INVALID, "sa is NULL");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    if (total == 0) return SA_OK;
    if (!pos_out) return set_err(SA_E_INVALID, "pos_out is NULL");
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(std::max<uint64_t>(n, 1), &c));
    DevBuf d_sa, d_lh, d_off, d_pos;
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_lh.alloc(align_up(2 * nq, 64) * 4));
    SA_TRY(d_off.alloc(align_up(nq + 1, 64) * 8));
    SA_TRY(d_pos.alloc(align_up(total, 64) * 4));
    SA_TRY(upload({{d_sa.p, src, n * 4}, {d_lh.p, lh.data(), 2 * nq * 4}}));
    uint64_t got = 0;
    SA_TRY(locate_device(c, n, d_sa.as<uint32_t>(), d_lh.as<uint32_t>(), d_lh.as<uint32_t>() + nq, nq, max_hits, flags,
                         d_off.as<uint64_t>(), d_pos.as<uint32_t>(), total, &got, nullptr));
    if (got != total)
        return set_err(SA_E_INTERNAL, "locate: the device counted %llu hits, the host %llu", (unsigned long long)got,
                       (unsigned long long)total);
    return copy_d2h(pos_out, d_pos.as<uint32_t>(), total, sa_width, nullptr);
}

}  // namespace sa

extern "C" {

int sa_locate_device(sa_context* ctx, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lo, const uint32_t* d_hi,
                     uint64_t nq, uint64_t max_hits, uint32_t flags, uint64_t* d_off, uint32_t* d_pos,
                     uint64_t pos_cap, uint64_t* total, void* stream) {
    return sa::locate_device(ctx, n, d_sa, d_lo, d_hi, nq, max_hits, flags, d_off, d_pos, pos_cap, total,
                             (hipStream_t)stream);
}

int sa_locate(const void* sa, uint64_t n, int sa_width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
              uint64_t max_hits, uint32_t flags, uint64_t* off_out, void* pos_out, uint64_t pos_cap) {
    return sa::locate_host(sa, n, sa_width, lo, hi, nq, max_hits, flags, off_out, pos_out, pos_cap);
}

}  // extern "C"

#endif   // __HIPCC__
