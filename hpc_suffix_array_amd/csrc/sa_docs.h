// sa_docs.h -- document collections over one suffix array: the document array,
// the document of a position, document frequency and document listing of SA
// intervals (sa_doc_array / sa_doc_of / sa_doc_frequency / sa_doc_list and
// their _device forms of include/sa_hip.h).
//
// A collection is a text of n bytes and D + 1 non-decreasing uint64 offsets
// doc_off with doc_off[0] = 0 and doc_off[D] = n; document d is the bytes
// [doc_off[d], doc_off[d + 1]).  doc(p) = the largest d with doc_off[d] <= p
// (never an empty document), DA[r] = doc(SA[r]), PRV[r] = 1 + the largest
// r' < r with DA[r'] == DA[r] (0: none).  The distinct documents of [lo, hi)
// are the ranks r in it with PRV[r] <= lo (Muthukrishnan), so
// df = #{ r in [lo, hi) : PRV[r] <= lo } is one streaming pass, and only the
// surviving ids are sorted.  The text is never read.
//
//   k_doc_map        doc(p) for an array of positions (the SA for the document
//                    array, any positions for sa_doc_of): doc_search over the
//                    boundaries, staged as uint32 in LDS when D <= kDocLdsDocs,
//                    read from global memory (L2-resident) otherwise.  It also
//                    writes the (document, rank) pairs the sort of PRV takes.
//   PRV              the context's LSD radix sort (sa_sort_pairs_device, stable)
//                    orders the ranks by document over doc_key_bits(D) key bits;
//                    k_doc_prev then writes prev[L[k]] = L[k - 1] + 1 where both
//                    have the same document.
//   k_doc_freq_group an interval of up to kDocGroupMax ranks is counted by a
//                    group of kDocGroup lanes, 16 queries per workgroup and
//                    step; the kernel writes every df[q] (0 for the others) and
//                    the number of chunks of each longer interval.
//   k_doc_freq_tiled a longer interval is cut into chunks of kDocTile ranks;
//                    the chunk numbers are summed (scan_i64) and a persistent
//                    grid takes chunk x of the sum, finds its query by binary
//                    search and adds its count into df[q].
//   listing          c[q] = min(df[q], max_docs) is summed into off; after the
//                    one host wait for the total, k_doc_fill_group / _long write
//                    DA[r] of the first c[q] qualifying ranks in rank order (a
//                    long interval is one workgroup's stream), and sa_locate.h's
//                    per-query sort orders each query's ids.
//
// The arithmetic (the boundary search, the PRV predicate, the capped count,
// the class and chunks of a query, the key width of D) compiles on the host:
// tests/cpp/docs_check.cpp checks it against brute force.
// Measurements: DESIGN.md section 19.
// The HIP part needs sa_host.h, sa_locate.h and sa_query.h (ListSort) before it.
#pragma once
#include <stdint.h>

#include "sa_locate.h"   // locate_count, locate_bits, locate_lower_bound

namespace sa {

constexpr uint32_t kDocNone = 0xFFFFFFFFu;       // = SA_DOC_NONE
constexpr uint32_t kDocTile = 2048;              // ranks per chunk of a long interval (= SA_DOC_TILE = _native.DOC_TILE)
constexpr uint32_t kDocGroup = 16;               // lanes that share a short interval
constexpr uint32_t kDocGroupMax = 256;           // the longest interval of the group class (= SA_DOC_GROUP_MAX)
constexpr uint32_t kDocLdsDocs = 8192;           // most documents whose boundaries are staged in LDS (= SA_DOC_LDS_DOCS)
constexpr uint64_t kDocMaxDocs = 0xFFFFFFFEull;  // D <= 2^32 - 2: every id is below SA_DOC_NONE

// doc(p): the largest d in [0, D) with off(d) <= p; 0 when there is none
// (off(0) = 0 in a collection).  Reads off(0 .. D - 1) only, whatever they hold.
template <class Off>
SA_HD uint32_t doc_search(const Off& off, uint64_t D, uint64_t p) {
    uint64_t a = 0, len = D;   // first d with off(d) > p
    while (len > 0) {
        const uint64_t half = len >> 1;
        if (off(a + half) <= p) {
            a += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return a ? (uint32_t)(a - 1) : 0u;
}

// rank r is the first of its document inside [lo, hi) (lo <= r)
SA_HD bool doc_first(uint32_t prv, uint64_t lo) { return (uint64_t)prv <= lo; }

// the listed documents of a query with df distinct ones (max_docs == 0: no cap)
SA_HD uint32_t doc_capped(uint64_t df, uint64_t max_docs) {
    return (uint32_t)(max_docs && df > max_docs ? max_docs : df);
}

// the class of an interval of `len` ranks (len = locate_count(lo, hi, n, 0), so
// an interval that breaks lo <= hi <= n is empty)
enum DocClass : uint32_t { kDocEmpty = 0, kDocGroupClass = 1, kDocTiledClass = 2 };
SA_HD uint32_t doc_class(uint64_t len) {
    return len == 0 ? kDocEmpty : len <= kDocGroupMax ? kDocGroupClass : kDocTiledClass;
}
// chunks of kDocTile ranks of a tiled interval, 0 for the other classes
SA_HD uint64_t doc_chunks(uint64_t len) {
    return doc_class(len) == kDocTiledClass ? (len + kDocTile - 1) / kDocTile : 0;
}

// key bits of the sort by document: the ids are below D; the radix sort takes at least one
SA_HD uint32_t doc_key_bits(uint64_t D) {
    const uint32_t b = locate_bits(D);
    return b ? b : 1u;
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

#include "sa_kernels.h"

namespace sa {

static_assert(kDocNone == SA_DOC_NONE && kDocTile == SA_DOC_TILE && kDocGroupMax == SA_DOC_GROUP_MAX &&
                  kDocLdsDocs == SA_DOC_LDS_DOCS,
              "the header's constants");
static_assert(kDocTile == 8 * kBlock && kWave % kDocGroup == 0, "8 ranks per lane and chunk");
constexpr uint32_t kDocGrid = 1024;       // workgroups of the grids of the forms that take no context

struct DocOffLds {
    const uint32_t* p;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return p[i]; }
};
struct DocOffGlobal {
    const uint64_t* __restrict__ p;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return p[i]; }
};
// the chunk sums: entry i of nq + 1
struct DocChunks {
    const int64_t* __restrict__ p;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return (uint64_t)p[i]; }
};

// doc(pos[i]) for i < count.  OF (sa_doc_of): a position >= n gives kDocNone;
// otherwise (the document array) it is clamped to n - 1 (n > 0).  da, rel
// (position - the document's offset) and keys / vals (the pairs (document, i)
// of the sort) are each written when given.
template <bool LDS, bool OF>
__global__ __launch_bounds__(kBlock) void k_doc_map(const uint32_t* __restrict__ pos, uint64_t count, uint64_t n,
                                                    const uint64_t* __restrict__ doc_off, uint64_t D,
                                                    uint32_t* __restrict__ da, uint32_t* __restrict__ rel,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    __shared__ uint32_t s_off[LDS ? kDocLdsDocs : 1];
    if constexpr (LDS) {
        for (uint32_t i = threadIdx.x; i < D; i += kBlock) s_off[i] = (uint32_t)std::min<uint64_t>(doc_off[i], n);
        __syncthreads();
    }
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kBlock) {
        uint64_t p = pos[i];
        uint32_t d = kDocNone, r = kDocNone;
        if (!OF || p < n) {
            if (!OF) p = std::min<uint64_t>(p, n - 1);
            if constexpr (LDS) {
                d = doc_search(DocOffLds{s_off}, D, p);
                r = (uint32_t)p - s_off[d];
            } else {
                d = doc_search(DocOffGlobal{doc_off}, D, p);
                if (rel) r = (uint32_t)(p - doc_off[d]);
            }
        }
        if (da) da[i] = d;
        if (rel) rel[i] = r;
        if (keys) {
            keys[i] = d;
            vals[i] = (uint32_t)i;
        }
    }
}

// ranks L[0, n) ordered by (document, rank): prev[L[k]] = L[k - 1] + 1 where both have the same document
__global__ __launch_bounds__(kBlock) void k_doc_prev(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ L,
                                                     uint64_t n, uint32_t* __restrict__ prev) {
    for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kBlock) {
        const uint32_t r = L[k];
        uint32_t v = 0;
        if (k > 0 && keys[k - 1] == keys[k]) v = L[k - 1] + 1u;
        if (r < n) prev[r] = v;   // holds: L is a permutation of [0, n)
    }
}

// sum over the kDocGroup lanes of a group
__device__ __forceinline__ uint32_t doc_group_sum(uint32_t x) {
#pragma unroll
    for (int o = kDocGroup / 2; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o, kDocGroup);
    return x;
}

// every df[q]: the count of a group-class interval, 0 for the others; ch[q + 1] = the chunks of a tiled one
__global__ __launch_bounds__(kBlock) void k_doc_freq_group(const uint32_t* __restrict__ prev, uint64_t n,
                                                           const uint32_t* __restrict__ lo,
                                                           const uint32_t* __restrict__ hi, uint64_t nq,
                                                           uint32_t* __restrict__ df, int64_t* __restrict__ ch) {
    constexpr uint32_t kPerWave = kWave / kDocGroup;
    const uint32_t lane = lane_id(), gl = lane % kDocGroup;
    if (blockIdx.x == 0 && threadIdx.x == 0) ch[0] = 0;
    for (uint64_t qw = ((uint64_t)blockIdx.x * kWaves + wave_id()) * kPerWave; qw < nq;
         qw += (uint64_t)gridDim.x * kWaves * kPerWave) {
        const uint64_t q = qw + lane / kDocGroup;
        const bool valid = q < nq;
        const uint64_t a = valid ? lo[q] : 0;
        const uint32_t len = valid ? locate_count(a, hi[q], n, 0) : 0u;
        uint32_t cnt = 0;
        if (doc_class(len) == kDocGroupClass)
            for (uint32_t i = gl; i < len; i += kDocGroup) cnt += doc_first(prev[a + i], a) ? 1u : 0u;
        cnt = doc_group_sum(cnt);
        if (valid && gl == 0) {
            df[q] = cnt;
            ch[q + 1] = (int64_t)doc_chunks(len);
        }
    }
}

// chunk x of the summed chunk numbers ch (nq + 1): its query by binary search, its count added into df
__global__ __launch_bounds__(kBlock) void k_doc_freq_tiled(const uint32_t* __restrict__ prev, uint64_t n,
                                                           const uint32_t* __restrict__ lo,
                                                           const uint32_t* __restrict__ hi, uint64_t nq,
                                                           const int64_t* __restrict__ ch, uint32_t* __restrict__ df) {
    const uint64_t total = (uint64_t)ch[nq];
    for (uint64_t x = blockIdx.x; x < total; x += gridDim.x) {
        // the first i with ch[i] >= x + 1 is in [1, nq]: ch[0] = 0, ch[nq] = total
        const uint64_t i = locate_lower_bound(DocChunks{ch}, 0, nq + 1, x + 1);
        if (i == 0 || i > nq) continue;
        const uint64_t q = i - 1;
        const uint64_t a = lo[q];
        const uint64_t len = locate_count(a, hi[q], n, 0);
        const uint64_t start = (x - (uint64_t)ch[q]) * kDocTile;
        const uint64_t end = std::min<uint64_t>(len, start + kDocTile);
        uint32_t cnt = 0;
        for (uint64_t k = start + threadIdx.x; k < end; k += kBlock) cnt += doc_first(prev[a + k], a) ? 1u : 0u;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) cnt += (uint32_t)__shfl_down((int)cnt, o, kWave);
        if (lane_id() == 0 && cnt) atomicAdd(&df[q], cnt);
    }
}

// c[q] into off[q + 1] (summed afterwards); words[0]: the tiled queries that list something
__global__ __launch_bounds__(kBlock) void k_doc_list_count(const uint32_t* __restrict__ df,
                                                           const uint32_t* __restrict__ lo,
                                                           const uint32_t* __restrict__ hi, uint64_t nq, uint64_t n,
                                                           uint64_t max_docs, uint64_t* __restrict__ off,
                                                           unsigned long long* __restrict__ words) {
    unsigned long long nl = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = doc_capped(df[q], max_docs);
        off[q + 1] = c;
        if (c && doc_class(locate_count(lo[q], hi[q], n, 0)) == kDocTiledClass) ++nl;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[0] = 0;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) nl += __shfl_down(nl, o, kWave);
    if (lane_id() == 0 && nl) atomicAdd(&words[0], nl);
}

// the group class: DA[r] of the first c[q] qualifying ranks, in rank order, to ids[off[q] ..)
__global__ __launch_bounds__(kBlock) void k_doc_fill_group(const uint32_t* __restrict__ da,
                                                           const uint32_t* __restrict__ prev, uint64_t n,
                                                           const uint32_t* __restrict__ lo,
                                                           const uint32_t* __restrict__ hi, uint64_t nq,
                                                           const uint64_t* __restrict__ off, uint32_t* __restrict__ ids) {
    constexpr uint32_t kPerWave = kWave / kDocGroup;
    const uint32_t lane = lane_id(), gl = lane % kDocGroup, shift = lane - gl;
    for (uint64_t qw = ((uint64_t)blockIdx.x * kWaves + wave_id()) * kPerWave; qw < nq;
         qw += (uint64_t)gridDim.x * kWaves * kPerWave) {
        const uint64_t q = qw + lane / kDocGroup;
        const bool valid = q < nq;
        const uint64_t a = valid ? lo[q] : 0;
        uint32_t len = valid ? locate_count(a, hi[q], n, 0) : 0u;
        const uint64_t base = valid ? off[q] : 0;
        const uint32_t c = valid ? (uint32_t)(off[q + 1] - base) : 0u;
        if (doc_class(len) != kDocGroupClass || c == 0) len = 0;
        uint32_t maxlen = len;   // over the wave's groups: the loop below is uniform
        maxlen = std::max(maxlen, (uint32_t)__shfl_xor((int)maxlen, 16, kWave));
        maxlen = std::max(maxlen, (uint32_t)__shfl_xor((int)maxlen, 32, kWave));
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < maxlen; i += kDocGroup) {
            const bool qual = i + gl < len && doc_first(prev[a + i + gl], a);
            const uint32_t gm = (uint32_t)(__ballot(qual) >> shift) & 0xFFFFu;
            const uint32_t slot = cnt + __popc(gm & ((1u << gl) - 1u));
            if (qual && slot < c) ids[base + slot] = da[a + i + gl];
            cnt += __popc(gm);
        }
    }
}

// the tiled class: one workgroup streams the interval, kDocTile ranks a step, until c[q] ids are written
__global__ __launch_bounds__(kBlock) void k_doc_fill_long(const uint32_t* __restrict__ da,
                                                          const uint32_t* __restrict__ prev, uint64_t n,
                                                          const uint32_t* __restrict__ lo,
                                                          const uint32_t* __restrict__ hi, uint64_t nq,
                                                          const uint64_t* __restrict__ off, uint32_t* __restrict__ ids) {
    __shared__ uint32_t s_tmp[kWaves];
    constexpr uint32_t kPer = kDocTile / kBlock;
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const uint64_t a = lo[q];
        const uint64_t len = locate_count(a, hi[q], n, 0);
        const uint64_t base = off[q];
        const uint32_t c = (uint32_t)(off[q + 1] - base);
        if (doc_class(len) != kDocTiledClass || c == 0) continue;   // uniform
        uint32_t done = 0;
        for (uint64_t i0 = 0; i0 < len && done < c; i0 += kDocTile) {
            const uint64_t k0 = i0 + (uint64_t)threadIdx.x * kPer;
            uint32_t bits = 0;
#pragma unroll
            for (uint32_t j = 0; j < kPer; ++j)
                if (k0 + j < len && doc_first(prev[a + k0 + j], a)) bits |= 1u << j;
            uint32_t tot = 0;
            uint32_t slot = done + block_exclusive_sum((uint32_t)__popc(bits), s_tmp, &tot);
            while (bits) {
                const uint32_t j = (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                if (slot < c) ids[base + slot] = da[a + k0 + j];
                ++slot;
            }
            done += tot;
        }
    }
}

// ---- device forms -----------------------------------------------------------
static int doc_check_D(uint64_t D) {
    if (D == 0) return set_err(SA_E_INVALID, "D is 0: a collection has at least one document");
    if (D > kDocMaxDocs) return set_err(SA_E_INVALID, "D too large");
    return SA_OK;
}
static int doc_check_out(const void* p, const char* name) {
    return ((uintptr_t)p & 3u) ? set_err(SA_E_INVALID, "%s is not 4-byte aligned", name) : SA_OK;
}

// positions -> documents, shared by the document array and sa_doc_of
template <bool OF>
static void doc_map_launch(uint32_t grid, hipStream_t s, const uint32_t* d_pos, uint64_t count, uint64_t n,
                           const uint64_t* d_doc_off, uint64_t D, uint32_t* d_da, uint32_t* d_rel, uint64_t* d_keys,
                           uint32_t* d_vals) {
    if (D <= kDocLdsDocs)
        hipLaunchKernelGGL((k_doc_map<true, OF>), dim3(grid), dim3(kBlock), 0, s, d_pos, count, n, d_doc_off, D, d_da,
                           d_rel, d_keys, d_vals);
    else
        hipLaunchKernelGGL((k_doc_map<false, OF>), dim3(grid), dim3(kBlock), 0, s, d_pos, count, n, d_doc_off, D, d_da,
                           d_rel, d_keys, d_vals);
}
static uint32_t doc_grid(uint64_t items, uint64_t per_group, uint64_t cap) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_group - 1) / per_group, cap));
}

// Host waits: none for DA alone; with PRV the radix sort's own (one).
// Temporaries with PRV: 24 n bytes (keys and values, in and out), stream-ordered.
static int doc_array_device(sa_context* c, uint64_t n, const uint32_t* d_sa, const uint64_t* d_doc_off, uint64_t D,
                            uint32_t* d_da, uint32_t* d_prev, hipStream_t s) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    SA_TRY(doc_check_D(D));
    if (!d_da && !d_prev) return set_err(SA_E_INVALID, "d_da and d_prev are both NULL");
    if (!d_doc_off) return set_err(SA_E_INVALID, "d_doc_off is NULL");
    if (n && !d_sa) return set_err(SA_E_INVALID, "d_sa is NULL");
    SA_TRY(doc_check_out(d_da, "d_da"));
    SA_TRY(doc_check_out(d_prev, "d_prev"));
    if (d_da && d_da == d_prev) return set_err(SA_E_INVALID, "d_da may not alias d_prev");
    SA_TRY(check_no_alias({d_da, d_prev}, {d_sa, d_doc_off}, "an output may not alias d_sa or d_doc_off"));
    if (n == 0) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    const uint32_t grid = doc_grid(n, (uint64_t)kBlock * 16, (uint64_t)c->cus * 8);
    if (!d_prev) {
        doc_map_launch<false>(grid, s, d_sa, n, n, d_doc_off, D, d_da, nullptr, nullptr, nullptr);
        SA_HIP(hipGetLastError());
        return SA_OK;
    }
    LocBuf tmp;   // keys in | keys out | values in | values out
    SA_TRY(tmp.alloc(n * 24, s));
    uint64_t* k_in = (uint64_t*)tmp.p;
    uint64_t* k_out = k_in + n;
    uint32_t* v_in = (uint32_t*)(k_out + n);
    uint32_t* v_out = v_in + n;
    doc_map_launch<false>(grid, s, d_sa, n, n, d_doc_off, D, d_da, nullptr, k_in, v_in);
    SA_HIP(hipGetLastError());
    SA_TRY(sa_sort_pairs_device(c, k_in, v_in, n, doc_key_bits(D), k_out, v_out, s));
    hipLaunchKernelGGL(k_doc_prev, dim3(doc_grid(n, kBlock, (uint64_t)c->cus * 16)), dim3(kBlock), 0, s,
                       (const uint64_t*)k_out, (const uint32_t*)v_out, n, d_prev);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// Host waits: none.
static int doc_of_device(const uint64_t* d_doc_off, uint64_t D, uint64_t n, const uint32_t* d_pos, uint64_t count,
                         uint32_t* d_doc, uint32_t* d_rel, hipStream_t s) {
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    SA_TRY(doc_check_D(D));
    if (!d_doc && !d_rel) return set_err(SA_E_INVALID, "d_doc and d_rel are both NULL");
    if (!d_doc_off) return set_err(SA_E_INVALID, "d_doc_off is NULL");
    if (count && !d_pos) return set_err(SA_E_INVALID, "d_pos is NULL");
    SA_TRY(doc_check_out(d_doc, "d_doc"));
    SA_TRY(doc_check_out(d_rel, "d_rel"));
    if (d_doc && d_doc == d_rel) return set_err(SA_E_INVALID, "d_doc may not alias d_rel");
    SA_TRY(check_no_alias({d_doc, d_rel}, {d_pos, d_doc_off}, "an output may not alias d_pos or d_doc_off"));
    if (count == 0) return SA_OK;
    doc_map_launch<true>(doc_grid(count, (uint64_t)kBlock * 16, kDocGrid), s, d_pos, count, n, d_doc_off, D, d_doc, d_rel,
                         nullptr, nullptr);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// Host waits: none.  Temporary: 8 (nq + 1) bytes (the chunk sums), stream-ordered.
// The work is the sum of the interval lengths at 4 bytes per rank.
static int doc_frequency_device(uint64_t n, const uint32_t* d_prev, const uint32_t* d_lo, const uint32_t* d_hi,
                                uint64_t nq, uint32_t* d_df, hipStream_t s) {
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (nq == 0) return SA_OK;
    if (n && !d_prev) return set_err(SA_E_INVALID, "d_prev is NULL");
    if (!d_lo) return set_err(SA_E_INVALID, "d_lo is NULL");
    if (!d_hi) return set_err(SA_E_INVALID, "d_hi is NULL");
    if (!d_df) return set_err(SA_E_INVALID, "d_df is NULL");
    SA_TRY(doc_check_out(d_df, "d_df"));
    SA_TRY(check_no_alias({d_df}, {d_prev, d_lo, d_hi}, "d_df may not alias an input"));
    LocBuf ch;
    SA_TRY(ch.alloc((nq + 1) * 8, s));
    hipLaunchKernelGGL(k_doc_freq_group, dim3(doc_grid(nq, kBlock / kDocGroup, 4 * kDocGrid)), dim3(kBlock), 0, s, d_prev,
                       n, d_lo, d_hi, nq, d_df, (int64_t*)ch.p);
    SA_HIP(hipGetLastError());
    SA_TRY(scan_i64<ScanSum>((int64_t*)ch.p + 1, nq, s));
    hipLaunchKernelGGL(k_doc_freq_tiled, dim3(kDocGrid), dim3(kBlock), 0, s, d_prev, n, d_lo, d_hi, nq,
                       (const int64_t*)ch.p, d_df);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// the checks of sa_doc_list_device, all before any HIP call
static int doc_list_check(const sa_context* c, uint64_t n, const uint32_t* d_da, const uint32_t* d_prev,
                          const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t flags, const uint64_t* d_off,
                          const uint32_t* d_docs, const uint64_t* total) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!total) return set_err(SA_E_INVALID, "total is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    SA_TRY(check_flags(flags, SA_DOC_RANK_ORDER));
    if (!d_off) return set_err(SA_E_INVALID, "d_off is NULL");
    if ((uintptr_t)d_off & 7u) return set_err(SA_E_INVALID, "d_off is not 8-byte aligned");
    SA_TRY(doc_check_out(d_docs, "d_docs"));
    if (nq) {
        if (n && !d_da) return set_err(SA_E_INVALID, "d_da is NULL");
        if (n && !d_prev) return set_err(SA_E_INVALID, "d_prev is NULL");
        if (!d_lo) return set_err(SA_E_INVALID, "d_lo is NULL");
        if (!d_hi) return set_err(SA_E_INVALID, "d_hi is NULL");
    }
    SA_TRY(check_no_alias({d_off, d_docs}, {d_da, d_prev, d_lo, d_hi}, "an output may not alias an input"));
    if (d_docs && (const void*)d_docs == (const void*)d_off) return set_err(SA_E_INVALID, "d_docs may not alias d_off");
    return SA_OK;
}

// Host waits: one for the total; when ids are written, sa_locate_device's own
// over the materialised ids (one: no query lists more than SA_LOCATE_TILE
// documents; more otherwise), or one at the end with SA_DOC_RANK_ORDER.
// Temporaries, stream-ordered: 4 nq (df) + 8 (nq + 1) (the chunk sums); when ids
// are sorted 4 bytes per listed id and 8 nq for their ranges.
static int doc_list_device(sa_context* c, uint64_t n, const uint32_t* d_da, const uint32_t* d_prev, const uint32_t* d_lo,
                           const uint32_t* d_hi, uint64_t nq, uint64_t max_docs, uint32_t flags, uint64_t* d_off,
                           uint32_t* d_docs, uint64_t docs_cap, uint64_t* total, hipStream_t s) {
    SA_TRY(doc_list_check(c, n, d_da, d_prev, d_lo, d_hi, nq, flags, d_off, d_docs, total));
    *total = 0;
    SA_HIP(hipSetDevice(c->device));
    if (nq == 0) return empty_csr(d_off, 0, s);
    uint64_t* h = host_u64<kHwDocs, 2>(c);
    {
        LocBuf w;   // the long queries (16 bytes) | df
        SA_TRY(w.alloc(16 + nq * 4, s));
        uint32_t* d_df = (uint32_t*)w.p + 4;
        SA_HIP(hipMemsetAsync(w.p, 0, 16, s));
        SA_TRY(doc_frequency_device(n, d_prev, d_lo, d_hi, nq, d_df, s));
        hipLaunchKernelGGL(k_doc_list_count, dim3(doc_grid(nq, kBlock, (uint64_t)c->cus * 8)), dim3(kBlock), 0, s,
                           (const uint32_t*)d_df, d_lo, d_hi, nq, n, max_docs, d_off, (unsigned long long*)w.p);
        SA_HIP(hipGetLastError());
        SA_TRY(scan_i64<ScanSum>(reinterpret_cast<int64_t*>(d_off) + 1, nq, s));
        SA_HIP(hipMemcpyAsync(h, d_off + nq, 8, hipMemcpyDeviceToHost, s));
        SA_HIP(hipMemcpyAsync(h + 1, w.p, 8, hipMemcpyDeviceToHost, s));
    }
    SA_HIP(host_sync(s));
    const uint64_t sum = h[0], n_long = h[1];
    *total = sum;
    SA_TRACE("doc list: nq %llu total %llu long %llu", (unsigned long long)nq, (unsigned long long)sum,
             (unsigned long long)n_long);
    if (!d_docs || sum > docs_cap || sum == 0) return SA_OK;
    const bool direct = (flags & SA_DOC_RANK_ORDER) != 0;
    if (!direct && sum > 0xFFFFFFFFull)
        return set_err(SA_E_INVALID, "%llu ids are more than 2^32 - 1: cap them with max_docs", (unsigned long long)sum);
    ListSort tmp;   // the ids in rank order, then sorted
    if (!direct) SA_TRY(tmp.alloc(sum, nq, s));
    uint32_t* d_ids = direct ? d_docs : tmp.items;
    hipLaunchKernelGGL(k_doc_fill_group, dim3(doc_grid(nq, kBlock / kDocGroup, (uint64_t)c->cus * 16)), dim3(kBlock), 0, s,
                       d_da, d_prev, n, d_lo, d_hi, nq, (const uint64_t*)d_off, d_ids);
    if (n_long)
        hipLaunchKernelGGL(k_doc_fill_long, dim3(doc_grid(nq, 1, (uint64_t)c->cus * 4)), dim3(kBlock), 0, s, d_da, d_prev,
                           n, d_lo, d_hi, nq, (const uint64_t*)d_off, d_ids);
    SA_HIP(hipGetLastError());
    if (direct) {
        SA_HIP(host_sync(s));
        return SA_OK;
    }
    // the ids are any 32-bit words to the sort: key bits for 2^32 values
    return tmp.sort(c, "doc list", "ids", sum, nq, 0, d_off, d_docs, docs_cap, 1ull << 32, s);
}

// ---- host in, host out, over the steps of sa_host.h ---------------------------
// the collection's offsets, checked in full
static int doc_check_offsets(const uint64_t* doc_off, uint64_t D, uint64_t n) {
    SA_TRY(doc_check_D(D));
    if (!doc_off) return set_err(SA_E_INVALID, "doc_off is NULL");
    if (doc_off[0] != 0) return set_err(SA_E_INVALID, "doc_off[0] is %llu, not 0", (unsigned long long)doc_off[0]);
    for (uint64_t d = 0; d < D; ++d)
        if (doc_off[d + 1] < doc_off[d])
            return set_err(SA_E_INVALID, "doc_off decreases at document %llu", (unsigned long long)d);
    if (doc_off[D] != n)
        return set_err(SA_E_INVALID, "doc_off ends at %llu, the text has %llu bytes", (unsigned long long)doc_off[D],
                       (unsigned long long)n);
    return SA_OK;
}

static int doc_array_host(const void* sa, uint64_t n, int sa_width, const uint64_t* doc_off, uint64_t D, void* da_out,
                          void* prev_out) {
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    SA_TRY(doc_check_offsets(doc_off, D, n));
    if (!da_out && !prev_out) return set_err(SA_E_INVALID, "da_out and prev_out are both NULL");
    if (da_out == prev_out) return set_err(SA_E_INVALID, "da_out may not alias prev_out");
    if (n == 0) return SA_OK;
    if (!sa) return set_err(SA_E_INVALID, "sa is NULL");
    if (da_out == sa || prev_out == sa || da_out == (const void*)doc_off || prev_out == (const void*)doc_off)
        return set_err(SA_E_INVALID, "an output may not alias sa or doc_off");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_sa, d_off, d_da, d_prev;
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_off.alloc((D + 1) * 8));
    if (da_out) SA_TRY(d_da.alloc(align_up(n, 64) * 4));
    if (prev_out) SA_TRY(d_prev.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{d_sa.p, src, n * 4}, {d_off.p, doc_off, (D + 1) * 8}}));
    SA_TRY(doc_array_device(c, n, d_sa.as<uint32_t>(), d_off.as<uint64_t>(), D, d_da.as<uint32_t>(),
                            d_prev.as<uint32_t>(), nullptr));
    if (da_out) SA_TRY(copy_d2h(da_out, d_da.as<uint32_t>(), n, sa_width, nullptr));
    if (prev_out) SA_TRY(copy_d2h(prev_out, d_prev.as<uint32_t>(), n, sa_width, nullptr));
    return SA_OK;
}

static int doc_of_host(const uint64_t* doc_off, uint64_t D, uint64_t n, const void* pos, uint64_t count, int width,
                       void* doc_out, void* rel_out) {
    SA_TRY(check_width(width));
    SA_TRY(check_n32(n));
    SA_TRY(doc_check_offsets(doc_off, D, n));
    if (!doc_out && !rel_out) return set_err(SA_E_INVALID, "doc_out and rel_out are both NULL");
    if (doc_out == rel_out) return set_err(SA_E_INVALID, "doc_out may not alias rel_out");
    if (count == 0) return SA_OK;
    if (!pos) return set_err(SA_E_INVALID, "pos is NULL");
    if (doc_out == pos || rel_out == pos || doc_out == (const void*)doc_off || rel_out == (const void*)doc_off)
        return set_err(SA_E_INVALID, "an output may not alias pos or doc_off");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_u32(pos, count, width, 0xFFFFFFFFull, "position", narrow, &src));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    DevBuf d_pos, d_off, d_doc, d_rel;
    SA_TRY(d_pos.alloc(align_up(count, 64) * 4));
    SA_TRY(d_off.alloc((D + 1) * 8));
    if (doc_out) SA_TRY(d_doc.alloc(align_up(count, 64) * 4));
    if (rel_out) SA_TRY(d_rel.alloc(align_up(count, 64) * 4));
    SA_TRY(upload({{d_pos.p, src, count * 4}, {d_off.p, doc_off, (D + 1) * 8}}));
    SA_TRY(doc_of_device(d_off.as<uint64_t>(), D, n, d_pos.as<uint32_t>(), count, d_doc.as<uint32_t>(),
                         d_rel.as<uint32_t>(), nullptr));
    if (doc_out) SA_TRY(copy_d2h(doc_out, d_doc.as<uint32_t>(), count, width, nullptr));
    if (rel_out) SA_TRY(copy_d2h(rel_out, d_rel.as<uint32_t>(), count, width, nullptr));
    return SA_OK;
}

static int doc_frequency_host(const void* prev, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                              uint64_t* df_out) {
    SA_TRY(check_width(width));
    SA_TRY(check_n32(n));
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    if (nq == 0) return SA_OK;
    if (!df_out) return set_err(SA_E_INVALID, "df_out is NULL");
    std::vector<uint32_t> lh;
    SA_TRY(pack_intervals(lo, hi, nq, n, 0, nullptr, lh));
    SA_TRY(check_no_alias({df_out}, {prev, lo, hi}, "df_out may not alias an input"));
    if (n == 0) {
        std::fill(df_out, df_out + nq, 0ull);
        return SA_OK;
    }
    if (!prev) return set_err(SA_E_INVALID, "prev is NULL");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_u32(prev, n, width, n, "PRV", narrow, &src));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    DevBuf d_prev, d_lh, d_df;
    SA_TRY(d_prev.alloc(align_up(n, 64) * 4));
    SA_TRY(d_lh.alloc(align_up(2 * nq, 64) * 4));
    SA_TRY(d_df.alloc(align_up(nq, 64) * 4));
    SA_TRY(upload({{d_prev.p, src, n * 4}, {d_lh.p, lh.data(), 2 * nq * 4}}));
    SA_TRY(doc_frequency_device(n, d_prev.as<uint32_t>(), d_lh.as<uint32_t>(), d_lh.as<uint32_t>() + nq, nq,
                                d_df.as<uint32_t>(), nullptr));
    return download_u64({{df_out, d_df.as<uint32_t>()}}, nq);
}

// the host has PRV, so it fills off_out and checks docs_cap before any device work, as sa_locate does
static int doc_list_host(const void* da, const void* prev, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi,
                         uint64_t nq, uint64_t max_docs, uint32_t flags, uint64_t* off_out, void* docs_out,
                         uint64_t docs_cap) {
    SA_TRY(check_width(width));
    SA_TRY(check_n32(n));
    if (nq > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "nq too large");
    SA_TRY(check_flags(flags, SA_DOC_RANK_ORDER));
    if (!off_out) return set_err(SA_E_INVALID, "off_out is NULL");
    off_out[0] = 0;
    if (nq == 0) return SA_OK;
    std::vector<uint32_t> lh;
    SA_TRY(pack_intervals(lo, hi, nq, n, 0, nullptr, lh));
    if (n && (!da || !prev)) return set_err(SA_E_INVALID, "da or prev is NULL");
    SA_TRY(check_no_alias({docs_out}, {da, prev, lo, hi, off_out}, "docs_out may not alias another array"));
    SA_TRY(check_no_alias({off_out}, {da, prev, lo, hi}, "off_out may not alias an input"));
    std::vector<uint32_t> nda, nprev;
    const void *sda = nullptr, *sprev = nullptr;
    SA_TRY(narrow_u32(da, n, width, kDocMaxDocs - 1, "DA", nda, &sda));
    SA_TRY(narrow_u32(prev, n, width, n, "PRV", nprev, &sprev));
    const uint32_t* p32 = (const uint32_t*)sprev;
    for (uint64_t q = 0; q < nq; ++q) {
        uint64_t df = 0;
        for (uint64_t r = lo[q]; r < hi[q]; ++r) df += doc_first(p32[r], lo[q]) ? 1u : 0u;
        off_out[q + 1] = off_out[q] + doc_capped(df, max_docs);
    }
    const uint64_t total = off_out[nq];
    if (!docs_out) return SA_OK;   // the sizing call: off_out is filled
    if (docs_cap < total)
        return set_err(SA_E_INVALID, "docs_cap %llu is below the %llu ids", (unsigned long long)docs_cap,
                       (unsigned long long)total);
    if (total == 0) return SA_OK;
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(std::max<uint64_t>(n, 1), &c));
    DevBuf d_da, d_prev, d_lh, d_off, d_docs;
    SA_TRY(d_da.alloc(align_up(n, 64) * 4));
    SA_TRY(d_prev.alloc(align_up(n, 64) * 4));
    SA_TRY(d_lh.alloc(align_up(2 * nq, 64) * 4));
    SA_TRY(d_off.alloc(align_up(nq + 1, 64) * 8));
    SA_TRY(d_docs.alloc(align_up(total, 64) * 4));
    SA_TRY(upload({{d_da.p, sda, n * 4}, {d_prev.p, sprev, n * 4}, {d_lh.p, lh.data(), 2 * nq * 4}}));
    uint64_t got = 0;
    SA_TRY(doc_list_device(c, n, d_da.as<uint32_t>(), d_prev.as<uint32_t>(), d_lh.as<uint32_t>(),
                           d_lh.as<uint32_t>() + nq, nq, max_docs, flags, d_off.as<uint64_t>(), d_docs.as<uint32_t>(), total,
                           &got, nullptr));
    if (got != total)
        return set_err(SA_E_INTERNAL, "doc list: the device counted %llu ids, the host %llu", (unsigned long long)got,
                       (unsigned long long)total);
    return copy_d2h(docs_out, d_docs.as<uint32_t>(), total, width, nullptr);
}

}  // namespace sa

extern "C" {

int sa_doc_array_device(sa_context* ctx, uint64_t n, const uint32_t* d_sa, const uint64_t* d_doc_off, uint64_t D,
                        uint32_t* d_da, uint32_t* d_prev, void* stream) {
    return sa::doc_array_device(ctx, n, d_sa, d_doc_off, D, d_da, d_prev, (hipStream_t)stream);
}

int sa_doc_of_device(const uint64_t* d_doc_off, uint64_t D, uint64_t n, const uint32_t* d_pos, uint64_t count,
                     uint32_t* d_doc, uint32_t* d_rel, void* stream) {
    return sa::doc_of_device(d_doc_off, D, n, d_pos, count, d_doc, d_rel, (hipStream_t)stream);
}

int sa_doc_frequency_device(uint64_t n, const uint32_t* d_prev, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq,
                            uint32_t* d_df, void* stream) {
    return sa::doc_frequency_device(n, d_prev, d_lo, d_hi, nq, d_df, (hipStream_t)stream);
}

int sa_doc_list_device(sa_context* ctx, uint64_t n, const uint32_t* d_da, const uint32_t* d_prev, const uint32_t* d_lo,
                       const uint32_t* d_hi, uint64_t nq, uint64_t max_docs, uint32_t flags, uint64_t* d_off,
                       uint32_t* d_docs, uint64_t docs_cap, uint64_t* total, void* stream) {
    return sa::doc_list_device(ctx, n, d_da, d_prev, d_lo, d_hi, nq, max_docs, flags, d_off, d_docs, docs_cap, total,
                               (hipStream_t)stream);
}

int sa_doc_array(const void* sa, uint64_t n, int sa_width, const uint64_t* doc_off, uint64_t D, void* da_out,
                 void* prev_out) {
    return sa::doc_array_host(sa, n, sa_width, doc_off, D, da_out, prev_out);
}

int sa_doc_of(const uint64_t* doc_off, uint64_t D, uint64_t n, const void* pos, uint64_t count, int width, void* doc_out,
              void* rel_out) {
    return sa::doc_of_host(doc_off, D, n, pos, count, width, doc_out, rel_out);
}

int sa_doc_frequency(const void* prev, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                     uint64_t* df_out) {
    return sa::doc_frequency_host(prev, n, width, lo, hi, nq, df_out);
}

int sa_doc_list(const void* da, const void* prev, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi,
                uint64_t nq, uint64_t max_docs, uint32_t flags, uint64_t* off_out, void* docs_out, uint64_t docs_cap) {
    return sa::doc_list_host(da, prev, n, width, lo, hi, nq, max_docs, flags, off_out, docs_out, docs_cap);
}

}  // extern "C"

#endif   // __HIPCC__
