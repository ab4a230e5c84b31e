// sa_host.h -- the host side of the host-pointer entry points, in one place:
// the staged copies between host memory and HBM, the process-wide context,
// the few steps every host form shares (argument checks, a width-8 SA
// narrowed to 32 bits, device buffers freed by scope, "upload these and
// wait", "download u32 results into the caller's u64 arrays"), and the host
// forms of the builder's own entry points (sa_build_ex, sa_check, sa_lcp).
// The host forms of the queries (sa_find.h, sa_match.h, sa_bwt.h,
// sa_locate.h) are written over the same steps.
//
// A host form reads: argument checks (all of them before the first HIP
// call), narrow, buffers as locals, then upload -> device form -> download,
// each through SA_TRY.  Nothing is freed by hand: a return anywhere is safe.
//
// Included by sa_build.hip below the device forms: it needs set_err, SA_HIP,
// SA_TRY, host_sync, align_up, ensure_capacity, build_device, check_device
// and lcp_device of that file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <vector>

namespace sa {

// ---------------------------------------------------------------------------
// Host <-> HBM copies of the host-pointer entry points (the reference's
// read_file / create path, utils.c:6-48, hands over pageable malloc memory).
// Pageable copies are staged by the HIP runtime one piece at a time; here a
// ring of pinned chunks is filled by several host threads while the DMA
// engine drains the previous chunk, so the PCIe link stays busy.  Memory the
// caller already pinned (hipHostMalloc / hipHostRegister) is copied directly.
// ---------------------------------------------------------------------------
constexpr size_t kStageChunk = 32ull << 20;
constexpr int kStageBufs = 3;

static bool host_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// memcpy of a large block by up to 8 threads (one core moves ~10 GB/s, the
// link ~50 GB/s)
static void par_memcpy(void* dst, const void* src, size_t bytes) {
    const size_t kPiece = 4ull << 20;
    const int th = (int)std::min<size_t>(8, (bytes + kPiece - 1) / kPiece);
    if (th <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (bytes + th - 1) / th;
    for (int t = 0; t < th; ++t) {
        const size_t a = (size_t)t * per, e = std::min(bytes, a + per);
        if (a >= e) break;
        pool.emplace_back([=] { std::memcpy((char*)dst + a, (const char*)src + a, e - a); });
    }
    for (auto& x : pool) x.join();
}

struct Staging {
    void* buf[kStageBufs] = {nullptr, nullptr, nullptr};
    hipEvent_t ev[kStageBufs] = {nullptr, nullptr, nullptr};
    int make() {
        for (int i = 0; i < kStageBufs; ++i) {
            if (hipHostMalloc(&buf[i], kStageChunk, hipHostMallocDefault) != hipSuccess ||
                hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                return set_err(SA_E_NOMEM, "pinned staging allocation failed");
            }
        }
        return SA_OK;
    }
    ~Staging() {
        for (int i = 0; i < kStageBufs; ++i) {
            if (buf[i]) hipHostFree(buf[i]);
            if (ev[i]) hipEventDestroy(ev[i]);
        }
    }
};

static int copy_h2d(void* d_dst, const void* h_src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return SA_OK;
    if (bytes <= kStageChunk || host_is_pinned(h_src)) {
        SA_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, s));
        return SA_OK;
    }
    Staging st;
    int rc = st.make();
    if (rc) return rc;
    size_t off = 0;
    for (int k = 0; off < bytes; ++k, off += kStageChunk) {
        const int b = k % kStageBufs;
        const size_t len = std::min(kStageChunk, bytes - off);
        if (k >= kStageBufs) SA_HIP(hipEventSynchronize(st.ev[b]));   // its previous DMA is done
        par_memcpy(st.buf[b], (const char*)h_src + off, len);
        SA_HIP(hipMemcpyAsync((char*)d_dst + off, st.buf[b], len, hipMemcpyHostToDevice, s));
        SA_HIP(hipEventRecord(st.ev[b], s));
    }
    SA_HIP(host_sync(s));
    return SA_OK;
}

// conv: 4 = raw u32 copy, 8 = widen u32 -> int64 into the host array
static int copy_d2h(void* h_dst, const uint32_t* d_src, uint64_t count, int width, hipStream_t s) {
    const size_t bytes = count * 4;
    if (count == 0) return SA_OK;
    if (width == 4 && (bytes <= kStageChunk || host_is_pinned(h_dst))) {
        SA_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, s));
        SA_HIP(host_sync(s));
        return SA_OK;
    }
    Staging st;
    int rc = st.make();
    if (rc) return rc;
    const uint64_t per = kStageChunk / 4;
    const uint64_t chunks = (count + per - 1) / per;
    auto issue = [&](uint64_t k) -> int {
        const int b = (int)(k % kStageBufs);
        const uint64_t a = k * per, len = std::min(per, count - a);
        SA_HIP(hipMemcpyAsync(st.buf[b], d_src + a, len * 4, hipMemcpyDeviceToHost, s));
        SA_HIP(hipEventRecord(st.ev[b], s));
        return SA_OK;
    };
    for (uint64_t k = 0; k < chunks && k + 1 < (uint64_t)kStageBufs; ++k)
        if ((rc = issue(k))) return rc;
    for (uint64_t k = 0; k < chunks; ++k) {
        const int b = (int)(k % kStageBufs);
        SA_HIP(hipEventSynchronize(st.ev[b]));
        if (k + kStageBufs - 1 < chunks && (rc = issue(k + kStageBufs - 1))) return rc;
        const uint64_t a = k * per, len = std::min(per, count - a);
        if (width == 4) {
            par_memcpy((uint32_t*)h_dst + a, st.buf[b], len * 4);
        } else {
            const uint32_t* src = (const uint32_t*)st.buf[b];
            int64_t* o = (int64_t*)h_dst + a;
            for (uint64_t i = 0; i < len; ++i) o[i] = src[i];
        }
    }
    return SA_OK;
}

// process-wide context for the host-pointer entry points (lazy, locked)
static std::mutex g_mu;
static sa_context* g_ctx = nullptr;

static int global_ctx(uint64_t n, sa_context** out) {
    if (!g_ctx) {
        int rc = sa_context_create(0, n, &g_ctx);
        if (rc) return rc;
    }
    *out = g_ctx;
    return ensure_capacity(g_ctx, n);
}

// ---------------------------------------------------------------------------
// the steps the host forms share
// ---------------------------------------------------------------------------
static int check_width(int sa_width) {
    return sa_width == 4 || sa_width == 8 ? SA_OK : set_err(SA_E_INVALID, "sa_width must be 4 or 8");
}
static int check_n32(uint64_t n) { return n > 0xFFFFFFFFull ? set_err(SA_E_INVALID, "n too large") : SA_OK; }
static int check_flags(uint32_t flags, uint32_t known) {
    return (flags & ~known) ? set_err(SA_E_INVALID, "unknown flags %#x", flags) : SA_OK;
}
static int check_exclusive(uint32_t flags, uint32_t a, uint32_t b, const char* name_a, const char* name_b) {
    return (flags & a) && (flags & b) ? set_err(SA_E_INVALID, "%s and %s exclude each other", name_a, name_b) : SA_OK;
}
// no output is an input; a NULL output is one the caller left out
static int check_no_alias(std::initializer_list<const void*> outs, std::initializer_list<const void*> ins,
                          const char* msg = "an output aliases an input") {
    for (const void* o : outs)
        for (const void* i : ins)
            if (o && o == i) return set_err(SA_E_INVALID, "%s", msg);
    return SA_OK;
}
static int check_distinct(std::initializer_list<const void*> outs, const char* msg = "two outputs are one buffer") {
    for (const void* const* a = outs.begin(); a != outs.end(); ++a)
        for (const void* const* b = outs.begin(); b != a; ++b)
            if (*a && *a == *b) return set_err(SA_E_INVALID, "%s", msg);
    return SA_OK;
}
// the forms that take no context ask for the device themselves, after every argument check
static int need_device() {
    return sa_device_count() > 0 ? SA_OK : set_err(SA_E_HIP, "no HIP device visible (libsa_hip needs an MI355X)");
}

// a width-8 array of m entries narrowed to 32 bits (entries outside [0, limit] rejected); *src = the 32-bit entries
static int narrow_u32(const void* a, uint64_t m, int width, uint64_t limit, const char* what,
                      std::vector<uint32_t>& narrow, const void** src) {
    *src = a;
    if (width == 8) {
        narrow.resize(m);
        const int64_t* w = (const int64_t*)a;
        for (uint64_t i = 0; i < m; ++i) {
            if (w[i] < 0 || (uint64_t)w[i] > limit) return set_err(SA_E_INVALID, "%s entry out of range", what);
            narrow[i] = (uint32_t)w[i];
        }
        *src = narrow.data();
    }
    return SA_OK;
}
static int narrow_sa(const void* sa, uint64_t n, int sa_width, std::vector<uint32_t>& narrow, const void** src) {
    return narrow_u32(sa, n, sa_width, n - 1, "SA", narrow, src);   // n == 0: no entry is looked at
}

// a device allocation freed by its scope (the sizes are the caller's: the
// kernels' word loads were written against each form's padding)
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) {
        if (hipMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return set_err(SA_E_NOMEM, "device allocation failed");
        }
        return SA_OK;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// upload these and wait (the null stream); an empty copy is skipped
struct H2D {
    void* dst;
    const void* src;
    size_t bytes;
};
static int upload(std::initializer_list<H2D> copies) {
    bool ok = true;
    for (const H2D& c : copies) ok = ok && copy_h2d(c.dst, c.src, c.bytes, nullptr) == SA_OK;
    if (!ok || host_sync(nullptr) != hipSuccess) return set_err(SA_E_HIP, "H2D copy failed: %s", g_err.c_str());
    return SA_OK;
}

// download count u32 results from each src and widen them into the caller's
// u64 array (a NULL dst is skipped); one wait, nothing written on failure
struct D2H {
    uint64_t* dst;
    const uint32_t* src;
};
static int download_u64(std::initializer_list<D2H> outs, uint64_t count) {
    std::vector<uint32_t> res(outs.size() * count);
    uint32_t* r = res.data();
    bool ok = true;
    for (const D2H& o : outs) {
        if (!o.dst) continue;
        ok = ok && hipMemcpyAsync(r, o.src, count * 4, hipMemcpyDeviceToHost, nullptr) == hipSuccess;
        r += count;
    }
    if (!ok || host_sync(nullptr) != hipSuccess)
        return set_err(SA_E_HIP, "search or D2H copy failed: %s", hipGetErrorString(hipGetLastError()));
    r = res.data();
    for (const D2H& o : outs) {
        if (!o.dst) continue;
        for (uint64_t q = 0; q < count; ++q) o.dst[q] = r[q];
        r += count;
    }
    return SA_OK;
}

// ---------------------------------------------------------------------------
// host in, host out: sa_build_ex, sa_check, sa_lcp
// ---------------------------------------------------------------------------
static int build_host(const uint8_t* text, uint64_t n, void* sa_out, int sa_width, const sa_opts* opts,
                      sa_stats* stats) {
    SA_TRY(check_width(sa_width));
    if (n && (!text || !sa_out)) return set_err(SA_E_INVALID, "NULL host pointer");
    if (n == 0) {
        if (stats) { std::memset(stats, 0, sizeof *stats); stats->n_kinds = SA_K_COUNT; }
        return SA_OK;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRACE("sa_build_ex n=%llu", (unsigned long long)n);
    SA_TRY(global_ctx(n, &c));
    DevBuf d_text, d_sa;
    SA_TRY(d_text.alloc(align_up(n, 256)));
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    // PCIe legs timed on the host clock (pinned staging overlaps host copies
    // with the DMA; sa_stats reports them apart from total_ms)
    using clock = std::chrono::steady_clock;
    using ms = std::chrono::duration<double, std::milli>;
    const auto t0 = clock::now();
    SA_TRY(copy_h2d(d_text.p, text, n, nullptr));
    SA_HIP(host_sync(nullptr));
    const double h2d = ms(clock::now() - t0).count();
    SA_TRY(build_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), nullptr, opts, stats));
    const auto t1 = clock::now();
    SA_TRY(copy_d2h(sa_out, d_sa.as<uint32_t>(), n, sa_width, nullptr));
    if (stats) {
        stats->h2d_ms = h2d;
        stats->d2h_ms = ms(clock::now() - t1).count();
    }
    return SA_OK;
}

// 1: the SA of the text, 0: not (a width-8 entry outside [0, n) included), < 0: an error
static int check_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width) {
    SA_TRY(check_width(sa_width));
    if (n == 0) return 1;
    if (!text || !sa) return set_err(SA_E_INVALID, "NULL host pointer");
    SA_TRY(check_n32(n));
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    if (narrow_sa(sa, n, sa_width, narrow, &src) != SA_OK) return 0;
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_text, d_sa;
    SA_TRY(d_text.alloc(align_up(n, 256)));
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}}));
    return check_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), nullptr);
}

static int lcp_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* lcp_out, uint64_t* lrs_len,
                    uint64_t* lrs_pos) {
    if (lrs_len) *lrs_len = 0;
    if (lrs_pos) *lrs_pos = 0;
    SA_TRY(check_width(sa_width));
    if (n == 0) return SA_OK;
    if (!text || !sa || !lcp_out) return set_err(SA_E_INVALID, "NULL host pointer");
    SA_TRY(check_n32(n));
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_text, d_sa, d_lcp;
    SA_TRY(d_text.alloc(align_up(n, 256)));
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(d_lcp.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}}));
    // the checker rejects a non-permutation before PHI would scatter through it
    const int valid = check_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), nullptr);
    if (valid == 0) return set_err(SA_E_INVALID, "not a valid suffix array of the text");
    if (valid != 1) return valid;
    Lrs lrs;
    const int rc = lcp_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_lcp.as<uint32_t>(), &lrs, nullptr);
    if (lrs_len) *lrs_len = lrs.len;
    if (lrs_pos) *lrs_pos = lrs.pos;
    if (rc) return rc;
    return copy_d2h(lcp_out, d_lcp.as<uint32_t>(), n, sa_width, nullptr);
}

}  // namespace sa
