// sa_bwt.h -- the Burrows-Wheeler transform of a text from its suffix array,
// with the primary index, the run count and the byte histogram
// (sa_bwt / sa_bwt_device of include/sa_hip.h), and the host drivers of the
// inverse suffix array (sa_inverse / sa_inverse_device, placed by the
// coalesced permutation of sa_permute.h as LCP's ISA + 1 is).
//
// bwt[r] = text[SA[r] - 1], text[n - 1] at the one rank with SA[r] == 0 (the
// primary index).  That is a random one-byte gather over the whole text: at
// n = 2^30 every gather is a line fetch from HBM (the text is four times the
// Infinity Cache), so the kernel is built for loads in flight, not for
// arithmetic:
//   * a workgroup takes kBwtTile = 4096 ranks per iteration: each lane reads
//     four 16-byte SA words (coalesced, 4 ranks each, one per quarter of the
//     tile) and has its 16 text gathers issued before the first byte is used;
//   * its four bytes of one SA word go out as one dword store;
//   * the grid is persistent: 8 workgroups of 256 threads per CU (8 waves per
//     SIMD, the registers allow it), striding over the tiles.
// The output may start at any byte: ranks [0, head) up to the first 4-byte
// boundary of d_bwt and the n mod 4 ranks after the last whole dword are
// written byte by byte by workgroup 0, so exactly d_bwt[0, n) is written.
// The SA words of a dword of output then sit at any 4-byte alignment; they are
// loaded as one 16-byte load of alignment 4 (global_load_dwordx4 takes it).
//
// STATS: a histogram in LDS (8 copies by lane, 257 words apart so that the
// copies of one byte lie in different banks: DNA's four hot bins would
// otherwise serialise 64 lanes on 4 addresses), flushed at the end with one
// 64-bit atomic per non-zero bin; runs counted as the ranks whose byte differs
// from the rank before (the previous byte of a lane's first rank is the lane
// below's last, a shuffle; for a wavefront's first lane it is gathered, at one
// address for the whole wavefront: one extra gather per 256 ranks), summed
// per workgroup into one atomic; the lane that sees SA[r] == 0 writes r.
// Without d_stats none of this is compiled in.
//
// An SA entry >= n (an invalid SA) reads text[n - 1]: no load leaves the
// buffers.
//
// Measured times, the cost of the statistics and the A/B run of the
// non-temporal SA loads and output stores (SA_BWT_NT=0 builds the plain
// variant): scripts/bench_bwt.py, DESIGN.md section 12, BASELINE.md "BWT".
//
// The HIP part needs sa_host.h before it (the host forms' staging, buffers,
// checks and the process-wide context), and with it sa_build.hip's set_err /
// SA_HIP / SA_TRY and the checker's permutation passes.
#pragma once
#include <stdint.h>

namespace sa {

// ranks one workgroup handles per iteration (= _native.BWT_TILE)
constexpr uint32_t kBwtTile = 4096;

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

#include "sa_kernels.h"

#ifndef SA_BWT_NT
#define SA_BWT_NT 1   // non-temporal SA loads and output stores (0: plain, A/B builds)
#endif

namespace sa {

constexpr int kBwtWords = 4;                    // 16-byte SA words per lane and iteration
constexpr uint32_t kBwtCopies = 8;              // LDS histogram copies
constexpr uint32_t kBwtCopyStride = 257;        // words between two copies (bank spread)
constexpr uint32_t kBwtGridPerCu = 8;           // workgroups per CU of the persistent grid
static_assert(kBwtTile == (uint32_t)kBlock * kBwtWords * 4, "tile = 256 lanes x 4 words x 4 ranks");
static_assert(SA_BWT_STATS == 258, "primary, runs, 256 counts");

typedef uint32_t bwt_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

// position of the byte that precedes suffix x in the text, its last byte for
// suffix 0: x - 1 wraps to 2^32 - 1 there and the minimum brings it to n - 1,
// as it does every entry > n of an invalid SA (1 <= n <= 2^32 - 1)
__device__ __forceinline__ uint32_t bwt_pos(uint32_t x, uint64_t n) {
    return std::min<uint32_t>(x - 1u, (uint32_t)(n - 1));
}

// the value is in its register here: the loads before this line are all
// issued before the first of them is waited for, and none of them sinks into
// the predicated code after it
#define SA_BWT_PIN(v) asm volatile("" : "+v"(v))

template <bool STATS>
__global__ __launch_bounds__(kBlock) void k_bwt(const uint8_t* __restrict__ text, uint64_t n,
                                                const uint32_t* __restrict__ sa, uint8_t* __restrict__ bwt,
                                                uint32_t head, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_h[STATS ? kBwtCopies * kBwtCopyStride : 1];
    __shared__ uint32_t s_runs;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = lane_id();
    uint32_t* my_h = s_h + (lane & (kBwtCopies - 1u)) * kBwtCopyStride;
    uint32_t runs = 0;
    if constexpr (STATS) {
        for (uint32_t i = tid; i < kBwtCopies * kBwtCopyStride; i += kBlock) s_h[i] = 0u;
        if (tid == 0) s_runs = 0u;
        __syncthreads();
    }
    const uint64_t nd = (n - head) >> 2;   // whole dwords of output after the head
    // the ranks outside the dwords, one lane each, byte stores
    if (blockIdx.x == 0) {
        const uint64_t tail0 = head + 4 * nd;
        const uint32_t edge = head + (uint32_t)(n - tail0);   // <= 3 + 3
        if (tid < edge) {
            const uint64_t r = tid < head ? tid : tail0 + (tid - head);
            const uint32_t x = sa[r];
            const uint8_t b = text[bwt_pos(x, n)];
            bwt[r] = b;
            if constexpr (STATS) {
                atomicAdd(&my_h[b], 1u);
                if (x == 0u) stats[0] = r;
                runs += r == 0 || text[bwt_pos(sa[r - 1], n)] != b;
            }
        }
    }
    const uint32_t* __restrict__ sa_b = sa + head;
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(bwt + head);
    const uint64_t tiles = (nd + kBlock * kBwtWords - 1) / (kBlock * kBwtWords);
    constexpr uint32_t TD = kBlock * kBwtWords;   // dwords of output per tile
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        // the tile's bases are uniform (scalar registers); a lane adds 32-bit offsets
        const uint64_t kb = t * TD;
        const uint32_t rem = (uint32_t)std::min<uint64_t>(nd - kb, TD);   // its dwords, >= 1
        const uint32_t* __restrict__ sa_t = sa_b + 4 * kb;
        uint32_t* __restrict__ out_t = out + kb;
        // No load below is predicated: a lane past the last dword reads the
        // last dword's words again (its store and its counts are predicated),
        // so that the 16 SA ranks and then the 16 gathers of a lane are all
        // issued before the first wait, with no branch between them.
        bwt_u32x4 x[kBwtWords];
        uint32_t px[kBwtWords];
#pragma unroll
        for (int j = 0; j < kBwtWords; ++j) {
            const uint32_t l = std::min<uint32_t>(tid + j * kBlock, rem - 1u);
            const bwt_u32x4* p = reinterpret_cast<const bwt_u32x4*>(sa_t + 4u * l);
#if SA_BWT_NT
            x[j] = __builtin_nontemporal_load(p);
#else
            x[j] = *p;
#endif
            if constexpr (STATS) {
                // the rank below the wavefront's first rank (its byte starts
                // the run compare): one address for the whole wavefront
                const uint32_t lw = std::min<uint32_t>(
                    (__builtin_amdgcn_readfirstlane(tid) & ~(uint32_t)(kWave - 1)) + j * kBlock, rem - 1u);
                px[j] = *(sa_t + 4u * lw - ((head | kb | lw) ? 1 : 0));
            }
        }
#pragma unroll
        for (int j = 0; j < kBwtWords; ++j) {
            SA_BWT_PIN(x[j]);
            if constexpr (STATS) SA_BWT_PIN(px[j]);
        }
        uint32_t b[kBwtWords][4];
        uint32_t pb[kBwtWords];
#pragma unroll
        for (int j = 0; j < kBwtWords; ++j) {
            b[j][0] = text[bwt_pos(x[j].x, n)];
            b[j][1] = text[bwt_pos(x[j].y, n)];
            b[j][2] = text[bwt_pos(x[j].z, n)];
            b[j][3] = text[bwt_pos(x[j].w, n)];
            pb[j] = STATS ? text[bwt_pos(px[j], n)] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kBwtWords; ++j) {
            SA_BWT_PIN(b[j][0]);
            SA_BWT_PIN(b[j][1]);
            SA_BWT_PIN(b[j][2]);
            SA_BWT_PIN(b[j][3]);
            if constexpr (STATS) SA_BWT_PIN(pb[j]);
        }
#pragma unroll
        for (int j = 0; j < kBwtWords; ++j) {
            const uint32_t l = tid + j * kBlock;
            const uint32_t w = b[j][0] | (b[j][1] << 8) | (b[j][2] << 16) | (b[j][3] << 24);
            if (l < rem) {
#if SA_BWT_NT
                __builtin_nontemporal_store(w, out_t + l);
#else
                out_t[l] = w;
#endif
            }
            if constexpr (STATS) {
                uint32_t prev = (uint32_t)__shfl_up((int)b[j][3], 1, kWave);
                if (lane == 0) prev = pb[j];
                if (l < rem) {
                    atomicAdd(&my_h[b[j][0]], 1u);
                    atomicAdd(&my_h[b[j][1]], 1u);
                    atomicAdd(&my_h[b[j][2]], 1u);
                    atomicAdd(&my_h[b[j][3]], 1u);
                    // rank 0 has no rank before it: it starts the first run
                    runs += ((head | kb | l) == 0 || prev != b[j][0]) + (b[j][1] != b[j][0]) + (b[j][2] != b[j][1]) +
                            (b[j][3] != b[j][2]);
                    const uint64_t r = head + 4 * (kb + l);
                    if (x[j].x == 0u) stats[0] = r;
                    if (x[j].y == 0u) stats[0] = r + 1;
                    if (x[j].z == 0u) stats[0] = r + 2;
                    if (x[j].w == 0u) stats[0] = r + 3;
                }
            }
        }
    }
    if constexpr (STATS) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) runs += (uint32_t)__shfl_down((int)runs, o, kWave);
        if (lane == 0 && runs) atomicAdd(&s_runs, runs);
        __syncthreads();
        if (tid == 0 && s_runs) atomicAdd(&stats[1], (unsigned long long)s_runs);
        uint64_t c = 0;
#pragma unroll
        for (uint32_t q = 0; q < kBwtCopies; ++q) c += s_h[q * kBwtCopyStride + tid];
        if (c) atomicAdd(&stats[2 + tid], (unsigned long long)c);
    }
}

// CUs of the current device (cached per device; 256 when the query fails)
static int bwt_cus() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return 256;
    }
    int cus = cached[dev].load(std::memory_order_relaxed);
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
            (void)hipGetLastError();
            cus = 256;
        }
        cached[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

static int bwt_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint8_t* d_bwt, uint64_t* d_stats,
                      hipStream_t s) {
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (n && (!d_text || !d_sa || !d_bwt)) return set_err(SA_E_INVALID, "NULL device pointer");
    if (n && ((const void*)d_bwt == (const void*)d_text || (const void*)d_bwt == (const void*)d_sa))
        return set_err(SA_E_INVALID, "d_bwt may not alias d_text or d_sa");
    if (d_stats) SA_HIP(hipMemsetAsync(d_stats, 0, SA_BWT_STATS * 8, s));
    if (n == 0) return SA_OK;
    const uint32_t head = (uint32_t)std::min<uint64_t>(n, (4 - ((uintptr_t)d_bwt & 3)) & 3);
    const uint64_t nd = (n - head) >> 2;
    const uint64_t tiles = (nd + kBlock * kBwtWords - 1) / (kBlock * kBwtWords);
    const uint32_t grid =
        (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)bwt_cus() * kBwtGridPerCu));
    if (d_stats)
        hipLaunchKernelGGL((k_bwt<true>), dim3(grid), dim3(kBlock), 0, s, d_text, n, d_sa, d_bwt, head,
                           reinterpret_cast<unsigned long long*>(d_stats));
    else
        hipLaunchKernelGGL((k_bwt<false>), dim3(grid), dim3(kBlock), 0, s, d_text, n, d_sa, d_bwt, head,
                           (unsigned long long*)nullptr);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// host in, host out (sa_bwt), over the steps of sa_host.h
static int bwt_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, uint8_t* bwt_out,
                    uint64_t* stats_out) {
    if (stats_out) std::memset(stats_out, 0, SA_BWT_STATS * 8);
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (n == 0) return SA_OK;
    if (!text || !sa || !bwt_out) return set_err(SA_E_INVALID, "NULL host pointer");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    SA_TRY(need_device());
    DevBuf d_text, d_sa, d_bwt, d_stats;
    SA_TRY(d_text.alloc(align_up(n, 256)));
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_bwt.alloc(align_up(n, 256)));
    SA_TRY(d_stats.alloc(SA_BWT_STATS * 8));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}}));
    SA_TRY(bwt_device(d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_bwt.as<uint8_t>(),
                      stats_out ? d_stats.as<uint64_t>() : nullptr, nullptr));
    if (hipMemcpyAsync(bwt_out, d_bwt.p, n, hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
        (stats_out &&
         hipMemcpyAsync(stats_out, d_stats.p, SA_BWT_STATS * 8, hipMemcpyDeviceToHost, nullptr) != hipSuccess) ||
        host_sync(nullptr) != hipSuccess)
        return set_err(SA_E_HIP, "BWT or D2H copy failed: %s", hipGetErrorString(hipGetLastError()));
    return SA_OK;
}

// ISA by the coalesced permutation (sa_check.h pass A's pairs under LCP's
// source name; k_perm_place's SUB = 1 stores r, not r + 1), the cursors
// checked as the checker's pass A checks them: the error word is 0 exactly
// when d_sa is a permutation of [0, n).  k_perm_place writes whole 16-byte
// groups only where four ranks are valid and the rest one by one, so nothing
// past d_isa[n - 1] is written; its 16-byte stores need the alignment.
static int inverse_device(sa_context* c, uint64_t n, const uint32_t* d_sa, uint32_t* d_isa, hipStream_t s) {
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (n == 0) return SA_OK;
    if (!d_sa || !d_isa) return set_err(SA_E_INVALID, "NULL device pointer");
    if ((const void*)d_sa == (const void*)d_isa) return set_err(SA_E_INVALID, "d_isa may not alias d_sa");
    if ((uintptr_t)d_isa & 15) return set_err(SA_E_INVALID, "d_isa must be 16-byte aligned");
    SA_HIP(hipSetDevice(c->device));
    SA_TRY(ensure_capacity(c, n));
    uint32_t* err = c->words + kPlaceErrWord;
    uint32_t bits = 0;   // the error bits of the last run
    for (uint32_t stripes : {kChkStripes, 1u}) {
        SA_HIP(hipMemsetAsync(err, 0, 4, s));
        SA_TRY(place_by_permutation<IsaSrc, 5, 1>(c, IsaSrc{{d_sa}}, n, d_isa, err, s, stripes));
        const PermPlan p = plan_check(n, kChkSubA);   // place_by_permutation's plan
        const BinStripes bs = plan_stripes(c, n, p, stripes);
        hipLaunchKernelGGL(k_chk_cursors,
                           dim3((uint32_t)std::min<uint64_t>(((uint64_t)p.nb1 * (p.nsub + 1) + kBlock - 1) / kBlock, 1024)),
                           dim3(kBlock), 0, s, (const uint32_t*)c->hist, (const uint32_t*)(c->hist + kCur2), n, p.s1,
                           p.s2, p.nb1, err, bs.st, chk_stride(p));
        SA_HIP(hipGetLastError());
        SA_READ(w, read_word(c, kPlaceErrWord, s));
        bits = *w;
        SA_TRACE("inverse (%u stripes asked, %u run): error bits %#x", stripes, bs.st, bits);
        if (!(bits & 128u)) break;   // else a stripe overflowed: again with one
    }
    if (bits) return set_err(SA_E_INVALID, "SA is not a permutation of [0, n) (error bits %#x)", bits);
    return SA_OK;
}

// host in, host out (sa_inverse), over the steps of sa_host.h
static int inverse_host(const void* sa, uint64_t n, int sa_width, void* isa_out) {
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (n == 0) return SA_OK;
    if (!sa || !isa_out) return set_err(SA_E_INVALID, "NULL host pointer");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_sa, d_isa;
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_isa.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{d_sa.p, src, n * 4}}));
    SA_TRY(inverse_device(c, n, d_sa.as<uint32_t>(), d_isa.as<uint32_t>(), nullptr));
    return copy_d2h(isa_out, d_isa.as<uint32_t>(), n, sa_width, nullptr);
}

}  // namespace sa

extern "C" {

int sa_bwt_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint8_t* d_bwt, uint64_t* d_stats,
                  void* stream) {
    return sa::bwt_device(d_text, n, d_sa, d_bwt, d_stats, (hipStream_t)stream);
}

int sa_bwt(const uint8_t* text, uint64_t n, const void* sa, int sa_width, uint8_t* bwt_out, uint64_t* stats_out) {
    return sa::bwt_host(text, n, sa, sa_width, bwt_out, stats_out);
}

int sa_inverse_device(sa_context* ctx, uint64_t n, const uint32_t* d_sa, uint32_t* d_isa, void* stream) {
    if (!ctx) return sa::set_err(SA_E_INVALID, "context is NULL");
    return sa::inverse_device(ctx, n, d_sa, d_isa, (hipStream_t)stream);
}

int sa_inverse(const void* sa, uint64_t n, int sa_width, void* isa_out) {
    return sa::inverse_host(sa, n, sa_width, isa_out);
}

}  // extern "C"

#endif   // __HIPCC__
