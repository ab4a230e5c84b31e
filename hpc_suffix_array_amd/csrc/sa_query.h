// sa_query.h -- what the query entry points share between their own kernels:
// block_sum_u64; the candidate tiles of sa_mem.h and sa_hamming.h (mem_tile_positions, mem_wave_turns,
// CandList); lists materialised, then sorted (k_list_ranges, sort_lists, ListSort).
// Needs sa_host.h and sa_locate.h before it, and sa_build.hip's scan_i64.
#pragma once
#include "sa_kernels.h"

namespace sa {

constexpr int kMemPer = 8;                               // candidates per lane
constexpr uint32_t kMemTile = kMemPer * kBlock;          // candidates per tile
constexpr uint32_t kMemGridPerCu = 4;                    // workgroups per CU of the persistent grids
static_assert(kMemTile == 2048, "16-bit slots, one flag byte per lane");

// words[k] += the workgroup's sum of v[k], k < N: one atomic per workgroup and word (every wavefront adding
// to the same two words, 8192 of them for a 1 MiB query, cost 0.1 ms); a sum of zero adds nothing
template <int N>
__device__ __forceinline__ void block_sum_u64(unsigned long long (&v)[N], unsigned long long* __restrict__ words) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __shfl_down(v[k], o, kWave);
    }
    __shared__ unsigned long long s_v[N][kWaves];
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_v[k][threadIdx.x / kWave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            unsigned long long sum = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) sum += s_v[k][w];
            if (sum) atomicAdd(&words[k], sum);
        }
    }
}

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

// Tile t of the candidate list: candidates [s, s + cnt); the positions whose list starts inside it are
// [q_lo, q_hi) (coff(q) in [s, s + cnt)), the empty ones among them included.
struct MemTile {
    uint64_t s, q_lo, q_hi;
    uint32_t cnt;
};

// The query position of each of the tile's candidates: s_pos[slot] for all kMemTile slots (what lies past cnt
// repeats the last position), and the calling lane's own kMemPer contiguous slots in pos.  s_q: 2 words, s_w:
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

// The nl slots the lanes listed, one per wavefront in turn: body(x, slot =
// slot_of(x), s_pos[slot], vals[slot]), all uniform over the wavefront.
template <class SlotOf, class Body>
__device__ __forceinline__ void mem_wave_turns(uint32_t nl, const SlotOf& slot_of, const uint32_t* s_pos,
                                               const uint32_t* __restrict__ vals, const Body& body) {
    for (uint32_t x = threadIdx.x / kWave; x < nl; x += kWaves) {
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot_of(x));
        body(x, slot, (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pos[slot]),
             (uint32_t)__builtin_amdgcn_readfirstlane((int)vals[slot]));
    }
}

// lists at off as intervals of one array: query q owns [off[q], off[q + 1])
__global__ __launch_bounds__(kBlock) void k_list_ranges(const uint64_t* __restrict__ off, uint64_t nq,
                                                        uint32_t* __restrict__ lo2, uint32_t* __restrict__ hi2) {
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock) {
        lo2[q] = (uint32_t)off[q];
        hi2[q] = (uint32_t)off[q + 1];
    }
}

// `total` items of nq lists in d_items, list q at [lo2[q], hi2[q]): every list ascending (flags: sa_locate_device's)
// into d_out, its offsets into d_off.  Host waits: locate_device_n's own.  what / unit: for the message.
static int sort_lists(sa_context* c, const char* what, const char* unit, uint64_t total, const uint32_t* d_items,
                      const uint32_t* d_lo2, const uint32_t* d_hi2, uint64_t nq, uint32_t flags, uint64_t* d_off,
                      uint32_t* d_out, uint64_t out_cap, uint64_t pos_n, hipStream_t s) {
    uint64_t got = 0;
    SA_TRY(locate_device_n(c, total, d_items, d_lo2, d_hi2, nq, 0, flags, d_off, d_out, out_cap, &got, s, pos_n));
    if (got != total)
        return set_err(SA_E_INTERNAL, "%s: %llu %s sorted of %llu", what, (unsigned long long)got, unit,
                       (unsigned long long)total);
    return SA_OK;
}

// lists materialised, then sorted: alloc (items | lo2 | hi2), the feature's kernels fill items at d_off, sort
struct ListSort {
    LocBuf tmp;
    uint32_t *items = nullptr, *lo2 = nullptr, *hi2 = nullptr;
    int alloc(uint64_t total, uint64_t nq, hipStream_t s) {
        const uint64_t b_items = align_up(total, 64) * 4;
        SA_TRY(tmp.alloc(b_items + 2 * nq * 4, s));
        items = (uint32_t*)tmp.p;
        lo2 = (uint32_t*)((uint8_t*)tmp.p + b_items);
        hi2 = lo2 + nq;
        return SA_OK;
    }
    int sort(sa_context* c, const char* what, const char* unit, uint64_t total, uint64_t nq, uint32_t flags,
             uint64_t* d_off, uint32_t* d_out, uint64_t out_cap, uint64_t pos_n, hipStream_t s) {
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nq + kBlock - 1) / kBlock, 256 * 8));
        hipLaunchKernelGGL(k_list_ranges, dim3(grid), dim3(kBlock), 0, s, (const uint64_t*)d_off, nq, lo2, hi2);
        SA_HIP(hipGetLastError());
        return sort_lists(c, what, unit, total, items, lo2, hi2, nq, flags, d_off, d_out, out_cap, pos_n, s);
    }
};

// the candidates of `rows` intervals in tiles of kMemTile: coff (rows + 1) | tile counts | candidates | flag bytes | extra
struct CandList {
    LocBuf buf;
    uint64_t cands = 0, tiles = 0;
    uint32_t grid = 0;   // of the persistent kernels over the tiles
    uint64_t* coff = nullptr;
    int64_t* tcnt = nullptr;   // per tile: the flagged candidates, summed by scan()
    uint32_t* cand = nullptr;
    uint8_t* flagb = nullptr;   // a byte per lane and tile
    void* extra = nullptr;      // extra_bytes, 4-byte aligned (kBlock % 4 == 0)
    // the `count` hits of [lo[q], hi[q]), q < rows, by locate_device (flags and host waits: its own).  No hit, or
    // more than max_candidates (0 = no cap): the empty answer in d_off (off_rows + 1), tiles stays 0, 0 / too_many.
    int fill(sa_context* c, const char* what, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lo,
             const uint32_t* d_hi, uint64_t rows, uint64_t count, uint64_t max_candidates, int too_many,
             uint64_t* d_off, uint64_t off_rows, uint32_t flags, uint64_t extra_bytes, hipStream_t s) {
        if (count == 0 || (max_candidates && count > max_candidates)) {
            SA_TRY(empty_csr(d_off, off_rows, s));
            return count ? too_many : SA_OK;
        }
        cands = count;
        tiles = (cands + kMemTile - 1) / kMemTile;
        grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)c->cus * kMemGridPerCu);
        SA_TRY(buf.alloc((rows + 1) * 8 + tiles * 8 + align_up(cands, 4) * 4 + tiles * kBlock + extra_bytes, s));
        coff = (uint64_t*)buf.p;
        tcnt = (int64_t*)(coff + rows + 1);
        cand = (uint32_t*)(tcnt + tiles);
        flagb = (uint8_t*)(cand + align_up(cands, 4));
        extra = flagb + tiles * kBlock;
        uint64_t got = 0;
        SA_TRY(locate_device(c, n, d_sa, d_lo, d_hi, rows, 0, flags, coff, cand, cands, &got, s));
        if (got != cands)
            return set_err(SA_E_INTERNAL, "%s: locate wrote %llu hits for %llu candidates", what, (unsigned long long)got,
                           (unsigned long long)cands);
        return SA_OK;
    }
    int scan(hipStream_t s) { return scan_i64<ScanSum>(tcnt, tiles, s); }
    // after scan(): the flagged candidates in all, through the pinned word h.  Host waits: one.
    int total(uint64_t* h, hipStream_t s, uint64_t* out) {
        SA_HIP(hipMemcpyAsync(h, tcnt + (tiles - 1), 8, hipMemcpyDeviceToHost, s));
        SA_HIP(host_sync(s));
        *out = *h;
        return SA_OK;
    }
};

}  // namespace sa
