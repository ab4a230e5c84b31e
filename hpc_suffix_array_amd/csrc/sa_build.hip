// sa_build.hip -- host driver of the MI355X rank-doubling suffix-array
// builder and the extended C ABI of include/sa_hip.h.
//
// Round structure (replaces build_suffix_array, manber_myers.c:81-133):
//   rank_1 = text + 1                                   (k_init_rank)
//   for h = 1, 2, 4, ...:                               (:97, 64-bit bound)
//     w  = bit width of D (ranks are 0..D)
//     P  = ceil(2w / 8) LSD passes over key (rank[i] << w) | rank[i+h]
//          pass 0 builds the key from ranks (the :116-124 update, fused)
//     D' = number of distinct keys                      (k_heads, k_scan_heads)
//     stop when D' == n                                 (:113)
//     rank[idx[p]] = dense rank of p                    (k_rerank, :101-110)
// The caller's SA buffer is one of the two index ping-pong buffers, chosen
// per round by the parity of P so the last pass writes the SA in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/sa_hip.h"

// alphabet kernel workgroups (overridable for A/B runs)
#ifndef SA_ALPHA_GRID
#define SA_ALPHA_GRID 2048
#endif

#include "sa_bucket.h"
#include "sa_check.h"
#include "sa_kernels.h"
#include "sa_lcp.h"
#include "sa_limits.h"
#include "sa_onesweep.h"
#include "sa_permute.h"
#include "sa_pivot.h"
#include "sa_split.h"
#include "sa_lsd.h"

namespace sa {

static thread_local std::string g_err;

static int set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define SA_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_err(SA_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),  \
                           __FILE__, __LINE__);                                              \
    } while (0)

// Every host wait of the library goes through these two (a stream sync, or
// a blocking copy): sa_host_syncs() reports their count, so a driver can
// show how many times a build stops the host (bench.py host_syncs_per_build).
static std::atomic<uint64_t> g_host_syncs{0};
static hipError_t host_sync(hipStream_t s) {
    g_host_syncs.fetch_add(1, std::memory_order_relaxed);
    return hipStreamSynchronize(s);
}
// a wait for the work up to an event: what was enqueued behind it runs on
static hipError_t host_sync_event(hipEvent_t e) {
    g_host_syncs.fetch_add(1, std::memory_order_relaxed);
    return hipEventSynchronize(e);
}
static hipError_t host_memcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    g_host_syncs.fetch_add(1, std::memory_order_relaxed);
    return hipMemcpy(dst, src, bytes, kind);
}

// propagate a non-zero status (variadic: template arguments carry commas)
#define SA_TRY(...)                      \
    do {                                 \
        const int rc_ = (__VA_ARGS__);   \
        if (rc_) return rc_;             \
    } while (0)

static bool trace_on() {
    static const bool on = std::getenv("SA_TRACE") != nullptr;
    return on;
}
#define SA_TRACE(...)                                   \
    do {                                                \
        if (trace_on()) {                               \
            std::fprintf(stderr, "[sa] " __VA_ARGS__);  \
            std::fputc('\n', stderr);                   \
        }                                               \
    } while (0)

// chunks of the chunked (tile-sequential) kernels: 4096 workgroups keep 16
// per CU in flight on the 256 CUs
#ifndef SA_MAX_CHUNKS
#define SA_MAX_CHUNKS 4096   // 16384 cut degenerate k_seg_write 317 -> 298 ms
#endif
constexpr uint32_t kMaxChunks = SA_MAX_CHUNKS;
// the one-workgroup chunk scans (k_seg_scan, k_scan_heads, k_scan_chunk_max)
// loop over blocks with a carry; the scratch arrays are sized by kMaxChunks
static_assert(kMaxChunks >= 1 && kMaxChunks <= (1u << 20), "chunk scratch sized for at most 2^20 chunks");
// sparse round-1 ranks when at most n / kSparseDiv suffixes stay unsorted
constexpr uint64_t kSparseDiv = 8;
constexpr int kEvPool = 256;
constexpr int kRoundEv = SA_MAX_ROUNDS + 1;   // round boundary events (Run::round_mark)
constexpr int kSyncEv = kEvPool + kRoundEv;   // recorded behind a read-back the host waits for (host_sync_event)

static uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

static uint32_t bit_width(uint64_t x) {
    uint32_t w = 0;
    while (x) { ++w; x >>= 1; }
    return w;
}

static Chunking plan_chunks(uint64_t n) {
    Chunking ch;
    ch.n = n;
    const uint64_t tiles = (n + kTile - 1) / kTile;
    uint64_t tpc = (tiles + kMaxChunks - 1) / kMaxChunks;
    if (tpc == 0) tpc = 1;
    ch.tiles_per_chunk = (uint32_t)tpc;
    ch.chunks = (uint32_t)std::max<uint64_t>(1, (tiles + tpc - 1) / tpc);
    return ch;
}

}  // namespace sa

namespace sa { struct DistState; }

struct sa_context {
    int device = 0;
    uint64_t cap = 0;      // rank / keys / vals_alt capacity (symbols)
    uint64_t cap_pad = 0;  // keys[0] / vals_alt capacity in elements (>= cap; padded first-pass segments)
    uint64_t ucap = 0;     // unsorted-set buffers capacity
    uint32_t* rank = nullptr;
    uint64_t* keys[2] = {nullptr, nullptr};
    uint32_t* vals_alt = nullptr;
    uint32_t* vals_u = nullptr;                 // sorted idx of an unsorted-set round
    uint32_t* u_pos[2] = {nullptr, nullptr};    // compacted unsorted set, ping-pong
    uint32_t* u_idx[2] = {nullptr, nullptr};
    uint32_t* u_g[2] = {nullptr, nullptr};
    uint32_t* u_gs[2] = {nullptr, nullptr};     // each set's group starts (pivot rounds; allocated at the first)
    uint64_t gscap = 0;
    uint64_t* keys_u = nullptr;                 // third key buffer (unsorted-set rounds)
    uint64_t kucap = 0;                         // keys_u capacity (items): ucap + the XQ regions' slack
    uint32_t* segx = nullptr;                   // second bucket pass, per-XCD queues (sa_split.h SegXq) + tables
    uint64_t segx_words = 0;
    uint32_t* os = nullptr;                     // onesweep ghist / digit bases / tickets
    uint32_t* lsd = nullptr;                    // k_lsd ghist [8][1024] | bases [8][1024] | tickets [8]
    uint32_t* lsdx = nullptr;                   // XQ k_lsd: per-queue counts [passes][8][1024] | bases [8][1024] | tickets
    uint32_t* segw = nullptr;                   // second bucket pass: per-segment cursors / bases / flags
    uint64_t* states = nullptr;                 // onesweep tile states [tiles][256]
    uint32_t epoch = 0;                         // onesweep state tag of the last pass
    uint64_t radix_passes = 0;                  // passes that took a tag since the context was made (SA_TRACE)
    int radix = 0;                              // 0 onesweep, 1 reduce-then-scan
    int cus = 256;                              // compute units (persistent grids)
    uint32_t* member = nullptr;                 // bitmap of round-1 unsorted positions
    uint32_t* hist = nullptr;      // 256 * kMaxChunks
    uint32_t* totals = nullptr;    // 256
    uint32_t* counts = nullptr;    // 4 * kMaxChunks (heads, u, uheads, last)
    uint32_t* words = nullptr;     // [0..2] = D, m, G; [3] = check error flags
    uint32_t* alpha = nullptr;     // 256 byte counts
    uint16_t* code = nullptr;      // 256 byte -> dense code 1..sigma
    uint32_t* host_words = nullptr;  // pinned, sa::kHostWords words: the regions are sa_limits.h's table (kHw*)
    hipEvent_t ev[sa::kEvPool + sa::kRoundEv + 1];   // Run timing pairs, the round boundaries, a read-back (kSyncEv)
    int ev_ready = 0;
    sa::DistState* dist = nullptr;   // range-partitioned build state (sa_dist.h)
    // sa_opts debug / tune fields of the current build (sa_build_device's
    // opts, or sa_context_set_debug for the sa_dist_* phases)
    uint32_t dbg = 0;
    int32_t span_extra = 0;
    int32_t tune = 0;
    bool dna = false;   // the text's alphabet is exactly {A, C, G, T} (k_split_text<.., DNA>)
    // the codes come from a sample of the text (build_packed): the first bucket
    // pass proves them, and round1_bucketed reports a refuted sample here
    bool alpha_prove = false;
    bool alpha_refuted = false;
    bool samples_pending = false;   // round 1 wrote no key1 samples (SegOut::samples = 0)
};

namespace sa {

// region R of the pinned words as the N 64-bit words its reader reads: the table holds exactly those
template <HwId R, int N> static uint64_t* host_u64(sa_context* c) {
    static_assert(hw(R).wide && hw(R).len == 2 * N, "sa_limits.h: a region is as long as what is read from it");
    return reinterpret_cast<uint64_t*>(c->host_words + hw(R).at);
}
static_assert(kLongRounds + 1 <= (int)hw(kHwLcpCounts).len && kMaxK <= (int)hw(kHwTail).len * 4, "sa_limits.h's regions");

// keys[0] / vals_alt elements for the padded first-pass segments of the
// bucketed round (sa_round1.h kPadMinN..kPadMaxN; their bound sums to < 1.1 n)
static uint64_t pad_capacity(uint64_t n) { return n + n / 8 + (1ull << 22); }

// keys[0] / vals_alt capacity (elements) of a context for n symbols
static uint64_t pad_elems(uint64_t n) {
    const uint64_t m = align_up(std::max<uint64_t>(n, 1), 64);
    return (n >= (1ull << 26) && n <= (1ull << 31)) ? align_up(pad_capacity(n), 64) : m;
}

// tile states for the widest digit (the bucketed first round's high pass
// uses up to 10 bits)
constexpr uint64_t kMaxRadix = 1024;
static uint64_t tile_states_bytes(uint64_t n) { return ((n + kTile - 1) / kTile + 1) * kMaxRadix * 8; }

// Device memory a context holds for n symbols: rank + 2 key + 1 index buffer
// (the reference schedule; keys[0] and the index buffer padded, pad_elems),
// plus 7 u32 arrays for the unsorted set (packed), keys_u with the per-XCD
// regions' slack (ensure_u_capacity), the group starts of pivot rounds
// (ensure_gs, 2 x (n/2 + 64) words) and the second pass's queue workspace
// (sa_round1.h: xq_words(1024) + 1032 + 2 x 8 x 2^19 bucket-table words at
// most) and the single-pass radix tile states.
static uint64_t ws_bytes(uint64_t n) {
    const uint64_t m = align_up(std::max<uint64_t>(n, 1), 64);
    const uint64_t ku_slack = n >= (1ull << 26) ? n / 16 + 8ull * 1024 * kXqSlack + 64 : 0;
    const uint64_t gs = 2 * (n / 2 + 64) * 4;
    const uint64_t segx = (xq_words(1024) + 1032 + 2ull * kXq * (1ull << 19)) * 4;
    return m * 4 + 2 * m * 8 + m * 4 + (pad_elems(n) - m) * 12 + 7 * m * 4 + (m + ku_slack) * 8 + m / 8 + gs +
           segx + tile_states_bytes(n) + (uint64_t)kRadix * kMaxChunks * 4 + 8192;
}

static void free_ctx_buffers(sa_context* c) {
    hipFree(c->rank);
    hipFree(c->keys[0]);
    hipFree(c->keys[1]);
    hipFree(c->vals_alt);
    hipFree(c->states);
    c->rank = nullptr;
    c->keys[0] = c->keys[1] = nullptr;
    c->vals_alt = nullptr;
    c->states = nullptr;
    c->cap = 0;
    c->cap_pad = 0;
}

static void free_u_buffers(sa_context* c) {
    hipFree(c->vals_u);
    hipFree(c->keys_u);
    hipFree(c->member);
    c->vals_u = nullptr;
    c->keys_u = nullptr;
    c->member = nullptr;
    for (int i = 0; i < 2; ++i) {
        hipFree(c->u_pos[i]);
        hipFree(c->u_idx[i]);
        hipFree(c->u_g[i]);
        hipFree(c->u_gs[i]);
        c->u_pos[i] = c->u_idx[i] = c->u_g[i] = c->u_gs[i] = nullptr;
    }
    c->gscap = 0;
    c->ucap = 0;
    c->kucap = 0;
}

// sa_opts debug / tune fields -> the context (NULL: production defaults)
static void set_debug(sa_context* c, const sa_opts* o) {
    c->dbg = o ? o->debug : 0u;
    c->span_extra = o ? o->span_extra : 0;
    c->tune = o ? o->tune : 0;
}

static int ensure_capacity(sa_context* c, uint64_t n) {
    if (n <= c->cap && c->rank) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    free_ctx_buffers(c);
    const uint64_t m = align_up(std::max<uint64_t>(n, 1), 64);
    // padded segments from 2^26 up to 2^31 suffixes (the bucketed round's
    // one-GPU maximum)
    const uint64_t mp = pad_elems(n);
    if (hipMalloc(&c->rank, m * 4) != hipSuccess || hipMalloc(&c->keys[0], mp * 8) != hipSuccess ||
        hipMalloc(&c->keys[1], m * 8) != hipSuccess || hipMalloc(&c->vals_alt, mp * 4) != hipSuccess ||
        hipMalloc(&c->states, tile_states_bytes(n)) != hipSuccess ||
        hipMemset(c->states, 0, tile_states_bytes(n)) != hipSuccess) {
        free_ctx_buffers(c);
        (void)hipGetLastError();
        return set_err(SA_E_NOMEM, "device allocation of %.2f GiB workspace failed",
                       (double)ws_bytes(n) / (1ull << 30));
    }
    c->cap = n;
    c->cap_pad = mp;
    SA_TRACE("workspace: rank %p keys0 %p keys1 %p vals_alt %p", (void*)c->rank, (void*)c->keys[0], (void*)c->keys[1],
             (void*)c->vals_alt);
    return SA_OK;
}

static int ensure_u_capacity(sa_context* c, uint64_t n) {
    if (n <= c->ucap && c->vals_u) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    free_u_buffers(c);
    const uint64_t m = align_up(std::max<uint64_t>(n, 1), 64) * 4;
    // keys_u also holds the second bucket pass's per-XCD regions (sa_split.h
    // SegXq): n items plus each (queue, digit) sub-region's slack, at most
    // n / 16 + 8 * 1024 * kXqSlack items (padded first-pass sizes only)
    const uint64_t ku = align_up(std::max<uint64_t>(n, 1), 64) +
                        (n >= (1ull << 26) ? n / 16 + 8ull * 1024 * kXqSlack + 64 : 0);
    bool ok = hipMalloc(&c->vals_u, m) == hipSuccess && hipMalloc(&c->keys_u, 8 * ku) == hipSuccess &&
              hipMalloc(&c->member, align_up(n, 1024) / 8) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i)
        ok = hipMalloc(&c->u_pos[i], m) == hipSuccess && hipMalloc(&c->u_idx[i], m) == hipSuccess &&
             hipMalloc(&c->u_g[i], m) == hipSuccess;
    if (!ok) {
        free_u_buffers(c);
        (void)hipGetLastError();
        return set_err(SA_E_NOMEM, "device allocation of the unsorted-set buffers failed");
    }
    c->ucap = n;
    c->kucap = ku;
    SA_TRACE("unsorted-set buffers: vals_u %p keys_u %p", (void*)c->vals_u, (void*)c->keys_u);
    return SA_OK;
}

// each unsorted set's group starts (pivot rounds, sa_pivot.h MODE 1): G <=
// m / 2 <= n / 2 words per set, allocated when a build first takes a pivot
// round (range builds never do)
static int ensure_gs(sa_context* c, uint64_t n) {
    if (n <= c->gscap && c->u_gs[0]) return SA_OK;
    for (int i = 0; i < 2; ++i) {
        hipFree(c->u_gs[i]);
        c->u_gs[i] = nullptr;
    }
    c->gscap = 0;
    const uint64_t w = n / 2 + 64;
    for (int i = 0; i < 2; ++i)
        if (hipMalloc(&c->u_gs[i], w * 4) != hipSuccess) {
            (void)hipGetLastError();
            for (int k = 0; k < 2; ++k) {
                hipFree(c->u_gs[k]);
                c->u_gs[k] = nullptr;
            }
            return set_err(SA_E_NOMEM, "group-start buffers (%llu words)", (unsigned long long)w);
        }
    c->gscap = n;
    return SA_OK;
}

// ensure_gs for a path that has an alternative: false (the HIP error and
// the message cleared) when the buffers cannot be allocated
static bool gs_available(sa_context* c, uint64_t n) {
    if (ensure_gs(c, n) == SA_OK) return true;
    (void)hipGetLastError();
    g_err.clear();
    SA_TRACE("group-start buffers unavailable: pivot rounds without tied blocks");
    return false;
}

// set i's group-start buffer when it holds an n-suffix build's groups
static uint32_t* gs_buf(const sa_context* c, uint64_t n, int i) { return n <= c->gscap ? c->u_gs[i] : nullptr; }

// One build's run context: the context, stream and statistics every build-side
// helper works on, with the per-launch HIP-event timing of sa_opts.profile
// (`on`).  Run{c, s, false, nullptr}: no timing, no statistics.
struct Run {
    sa_context* c;
    hipStream_t s;
    bool on;
    sa_stats* st;
    // algorithmic bytes moved by a kind of launch
    void bytes(int k, uint64_t b) {
        if (st) st->kern_bytes[k] += b;
    }
    int used = 0;
    int kind[kEvPool / 2];
    void begin(int k) {
        if (!on) return;
        if (used >= kEvPool / 2) flush();
        kind[used] = k;
        hipEventRecord(c->ev[2 * used], s);
    }
    void end() {
        if (!on) return;
        hipEventRecord(c->ev[2 * used + 1], s);
        ++used;
    }
    // round boundaries: one event before the first round and one after each,
    // read when the build has finished (round_times), so no round waits for
    // the GPU to drain before the next one is launched
    int nr = 0;
    uint64_t mark_bytes[kRoundEv] = {};   // the stats' algorithmic bytes at each boundary
    void round_mark() {
        if (nr < kRoundEv) {
            hipEventRecord(c->ev[kEvPool + nr], s);
            uint64_t b = 0;
            if (st)
                for (int k = 0; k < SA_K_COUNT; ++k) b += st->kern_bytes[k];
            mark_bytes[nr] = b;
        }
        ++nr;
    }
    // withdraw the last mark (the round it closed goes on after all); the
    // next round_mark records its event again
    void round_unmark() {
        if (nr > 0) --nr;
    }
    void round_times() {
        const int last = std::min(nr, kRoundEv) - 1;
        if (!st || last < 1) return;
        hipEventSynchronize(c->ev[kEvPool + last]);
        for (int r = 0; r < last && r < st->rounds; ++r) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, c->ev[kEvPool + r], c->ev[kEvPool + r + 1]);
            st->round_ms[r] = ms;
            st->round_bytes[r] = mark_bytes[r + 1] - mark_bytes[r];
        }
    }
    void flush() {
        if (!on || used == 0) return;
        hipEventSynchronize(c->ev[2 * used - 1]);
        for (int i = 0; i < used; ++i) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]);
            if (st) {
                st->kern_ms[kind[i]] += ms;
                st->kern_launches[kind[i]] += 1;
            }
        }
        used = 0;
    }
};

// owned HIP events (destroyed on every return path)
struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    int make() {
        for (auto& x : e)
            if (hipEventCreate(&x) != hipSuccess) return set_err(SA_E_HIP, "hipEventCreate failed");
        return SA_OK;
    }
    ~Events() {
        for (auto& x : e)
            if (x) hipEventDestroy(x);
    }
};

static float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, b);
    return ms;
}

// The read-back of a few words: `bytes` from d_src into the pinned words at
// `at`, and the host waits for them.  Returns them, or nullptr (the error set).
static const uint32_t* read_back(sa_context* c, uint32_t at, const void* d_src, size_t bytes, hipStream_t s) {
    uint32_t* const h = c->host_words + at;
    hipError_t e = hipMemcpyAsync(h, d_src, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = host_sync(s);
    if (e == hipSuccess) return h;
    set_err(SA_E_HIP, "read-back of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return nullptr;
}
// the first `bytes` of words[], or words[k] alone, into their mirror (kHwWords; indexed by the k*Word names)
static const uint32_t* read_words(sa_context* c, size_t bytes, hipStream_t s) { return read_back(c, 0, c->words, bytes, s); }
static const uint32_t* read_word(sa_context* c, int k, hipStream_t s) { return read_back(c, k, c->words + k, 4, s); }
#define SA_READ(var, ...)                         \
    const uint32_t* const var = (__VA_ARGS__);    \
    if (!var) return SA_E_HIP

// the D, m, G totals of a set of suffixes: distinct keys (group heads), the
// unsorted suffixes left and their groups
struct SetTotals {
    uint64_t D = 0, m = 0, G = 0;
};
static SetTotals totals_of(const uint32_t* w) { return SetTotals{w[kDWord], w[kMWord], w[kGWord]}; }
static SetTotals operator+(const SetTotals& a, const SetTotals& b) { return SetTotals{a.D + b.D, a.m + b.m, a.G + b.G}; }

// single-pass (onesweep) scratch: ghist[8][256] | base[8][256] | tickets[8]
static uint32_t* os_ghist(sa_context* c) { return c->os; }
static uint32_t* os_base(sa_context* c) { return c->os + kMaxPasses * kRadix; }
static uint32_t* os_tickets(sa_context* c) { return c->os + 2 * kMaxPasses * kRadix; }

// zero the global histograms and tile tickets of the next sort
static int onesweep_prepare(sa_context* c, hipStream_t s) {
    SA_HIP(hipMemsetAsync(c->os, 0, (2 * kMaxPasses * kRadix + kMaxPasses) * 4, s));
    return SA_OK;
}

static uint32_t next_epoch(sa_context* c, hipStream_t s) {
    ++c->radix_passes;
    if (++c->epoch > kEpochMask) {
        SA_TRACE("epoch wrap: %llu bytes of tile states cleared before radix pass %llu of the context",
                 (unsigned long long)tile_states_bytes(c->cap), (unsigned long long)c->radix_passes);
        hipMemsetAsync(c->states, 0, tile_states_bytes(c->cap), s);
        c->epoch = 1;
    }
    return c->epoch;
}

// pass p of a sort (its digit bases and ticket in the onesweep scratch)
template <class Src, int RBITS = 8>
static void onesweep_pass(Run& r, const Src& src, uint64_t n, uint32_t shift, uint32_t nbits, uint32_t p,
                          uint64_t* out_keys, uint32_t* out_vals) {
    sa_context* const c = r.c;
    const uint64_t tiles = (n + kTile - 1) / kTile;
    const uint32_t epoch = next_epoch(c, r.s);
    // 1024 x 4: 16 waves per tile, 2 workgroups (32 waves) per CU -- the
    // fastest shape in microbench.hip (r01: 10.4 ms per 2^30-pair pass)
    static_assert(kOsBlock * kOsItems == kTile, "tile states are sized for kTile");
    hipLaunchKernelGGL((k_onesweep<Src, kOsBlock, kOsItems, RBITS>), dim3((uint32_t)tiles), dim3(kOsBlock), 0, r.s, src,
                       n, shift, nbits, (const uint32_t*)(os_base(c) + p * kRadix), c->states, os_tickets(c) + p, epoch,
                       out_keys, out_vals, c->words + kLookbackWord);
}

// the buffers of a sort: the sorted idx land in vals_final, the pairs
// ping-pong through vals_other and the two key buffers
struct SortBufs {
    uint32_t *vals_final, *vals_other;
    uint64_t *kb0, *kb1;
};
struct Sorted {
    uint64_t* keys = nullptr;   // the key buffer that holds the sorted keys
    uint32_t passes = 0;
};
// hist0_ready: the first source's histograms are already computed (per chunk
// for the reduce-then-scan sort; global, after onesweep_prepare, otherwise).
// usort: an unsorted-set sort, accounted apart from the full-n passes
struct SortFlags {
    bool hist0_ready = false, usort = false;
};

// Stable LSD sort of ch.n (key, idx) pairs over key bits [0, bits): the first
// pass generates pairs from `first`, later passes read the ping-pong buffers.
template <class Src>
static int radix_sort(Run& r, const Src& first, uint64_t first_bytes, const Chunking& ch, uint32_t bits,
                      const SortBufs& b, Sorted* out, SortFlags f = SortFlags{}) {
    sa_context* const c = r.c;
    const uint32_t P = (bits + 7) / 8;
    if (P > kMaxPasses) return set_err(SA_E_INTERNAL, "%u radix passes", P);
    const int k_hist = f.usort ? SA_K_SORT_U : SA_K_HIST_FIRST;
    uint32_t* vb[2];
    vb[(P - 1) & 1] = b.vals_final;
    vb[P & 1] = b.vals_other;
    uint64_t* kb[2] = {b.kb0, b.kb1};
    out->keys = kb[(P - 1) & 1];
    out->passes = P;
    if (c->radix == 0) {
        const uint64_t n = ch.n;
        if (!f.hist0_ready) {
            SA_TRY(onesweep_prepare(c, r.s));
            r.begin(k_hist);
            const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, 2048);
            hipLaunchKernelGGL(k_global_hist<Src>, dim3(grid), dim3(kBlock), 0, r.s, first, n, P, os_ghist(c),
                               bits >= 64 ? ~0ull : (1ull << bits) - 1ull);
            r.end();
            r.bytes(k_hist, first_bytes);
        }
        r.begin(SA_K_SCAN);
        hipLaunchKernelGGL(k_digit_base, dim3(P), dim3(kBlock), 0, r.s, (const uint32_t*)os_ghist(c), os_base(c));
        r.end();
    }
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t shift = 8 * p;
        const uint32_t nbits = std::min<uint32_t>(8, bits - shift);
        const int kh = f.usort || !p ? k_hist : SA_K_HIST_KEYS;
        const int ks = f.usort ? SA_K_SORT_U : p ? SA_K_SCATTER_KEYS : SA_K_SCATTER_FIRST;
        const uint64_t in_bytes = p ? 12 * ch.n : first_bytes;
        auto pass = [&](const auto& src) {
            using S = std::decay_t<decltype(src)>;
            if (c->radix == 0) {
                r.begin(ks);
                onesweep_pass(r, src, ch.n, shift, nbits, p, kb[p & 1], vb[p & 1]);
                r.end();
                r.bytes(ks, in_bytes + 12 * ch.n);
                return;
            }
            // reduce-then-scan: chunk histograms, their scan, the scatter
            if (p || !f.hist0_ready) {
                r.begin(kh);
                hipLaunchKernelGGL(sa::k_hist<S>, dim3(ch.chunks), dim3(kBlock), 0, r.s, src, ch, shift,
                                   (1u << nbits) - 1u, c->hist);
                r.end();
                r.bytes(kh, in_bytes);
            }
            r.begin(SA_K_SCAN);
            hipLaunchKernelGGL(k_scan_rows, dim3(kRadix), dim3(kBlock), 0, r.s, c->hist, ch.chunks, c->totals);
            r.end();
            r.begin(ks);
            hipLaunchKernelGGL(k_scatter<S>, dim3(ch.chunks), dim3(kBlock), 0, r.s, src, ch, shift, nbits,
                               (const uint32_t*)c->hist, (const uint32_t*)c->totals, kb[p & 1], vb[p & 1]);
            r.end();
            r.bytes(SA_K_SCAN, 2ull * 4 * kRadix * ch.chunks);
            r.bytes(ks, in_bytes + 12ull * ch.n);
        };
        if (p == 0) pass(first);
        else pass(SrcKeys{kb[(p - 1) & 1], vb[(p - 1) & 1]});
    }
    SA_HIP(hipGetLastError());
    return SA_OK;
}

#include "sa_round1.h"

static void record_round(sa_stats* st, float ms, uint64_t D, uint32_t P, uint64_t sorted_n, uint64_t h) {
    if (!st) return;
    const int r = st->rounds;
    if (r < SA_MAX_ROUNDS) {
        st->round_ms[r] = ms;
        st->distinct[r] = D;
        st->passes[r] = (int32_t)P;
        st->sorted_n[r] = sorted_n;
        st->prefix_len[r] = h;
    }
    // B_j = n_j (3 rb + 2 S (P_j + 1)), rb = 4, S = 12
    st->model_bytes += sorted_n * (3ull * 4 + 2ull * 12 * (P + 1));
    st->rounds++;
}

// ---------------------------------------------------------------------------
// reference schedule: manber_myers.c:88-125 round for round
// ---------------------------------------------------------------------------
// the re-rank as a permutation (sa_permute.h) from this many suffixes; below
// it rank[] stays inside the L2s and one random scatter (k_rerank) is cheaper
// (SA_DEBUG_PERM_ALWAYS: from any n, for tests at small n)
constexpr int kPermErrWord = 13;
static uint64_t perm_min_n(const sa_context* c) { return (c->dbg & SA_DEBUG_PERM_ALWAYS) ? 1ull : (1ull << 22); }

// bin shifts of a permutation with 2^b1 first-level bins and sub-bins of 2^s2
// (the re-rank's; the checker's and the LCP's passes choose theirs)
static PermPlan plan_check(uint64_t n, uint32_t s2, uint32_t b1 = 8) {
    PermPlan p;
    const uint32_t lg = bit_width(n > 1 ? n - 1 : 1);   // ceil(log2 n)
    p.s2 = s2;
    p.s1 = std::max<uint32_t>(s2, lg > b1 ? lg - b1 : 0);
    p.nb1 = (uint32_t)((n + (1ull << p.s1) - 1) >> p.s1);
    p.nsub = 1u << (p.s1 - p.s2);
    p.tpb = (uint32_t)(((1ull << p.s1) + kPermBlock * kPermItems - 1) / (kPermBlock * kPermItems));
    return p;
}
static PermPlan plan_perm(uint64_t n) { return plan_check(n, kPermSub); }

// rank[idx[p]] = dense rank of sorted position p, through the two key
// buffers (the sorted keys are read by the first step and then free)
// first-level tiles of the permutation and their head offsets (k_tile_heads)
constexpr uint64_t kPermTile = (uint64_t)kPermBlock * kPermItems;
static_assert((kPermTile & (kPermTile - 1)) == 0, "power-of-two first-level tiles");
static uint32_t* perm_tile_off(sa_context* c) { return c->hist + ((uint64_t)kRadix * kMaxChunks) / 2; }
// tickets of the persistent permutation kernels: below the re-rank's tile offsets in hist
static uint32_t* perm_tickets(sa_context* c) { return c->hist + ((uint64_t)kRadix * kMaxChunks) / 2 - 64; }

static int rerank_permute(Run& r, uint64_t* sorted, const uint32_t* d_sa, const Chunking& ch, uint32_t kshift = 0,
                          NextHist nh = NextHist{}) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    const uint64_t n = ch.n;
    const PermPlan p = plan_perm(n);
    const uint64_t half = (uint64_t)kRadix * kMaxChunks / 2;   // cursors below, tile offsets above
    if (p.nb1 > 256 || p.nsub > kPermMaxSub || 256ull + (uint64_t)p.nb1 * p.nsub > half ||
        (n + kPermTile - 1) / kPermTile > half)
        return set_err(SA_E_INTERNAL, "permutation plan out of range (n=%llu)", (unsigned long long)n);
    uint64_t* other = sorted == c->keys[0] ? c->keys[1] : c->keys[0];
    uint32_t* cur1 = c->hist;          // the chunk histograms are free after the sort
    uint32_t* cur2 = c->hist + 256;
    SA_HIP(hipMemsetAsync(c->hist, 0, (256ull + (uint64_t)p.nb1 * p.nsub) * 4, s));
    r.begin(SA_K_RERANK);
    const uint32_t tiles = (uint32_t)((n + kPermTile - 1) / kPermTile);
    const uint32_t* toff = perm_tile_off(c);
    if (kshift)   // packed (key << kshift | idx) items
        hipLaunchKernelGGL((k_perm_rank<kPermBlock, kPermItems, true>), dim3(tiles), dim3(kPermBlock), 0, s,
                           (const uint64_t*)sorted, d_sa, n, toff, p.s1, kshift, cur1, other);
    else
        hipLaunchKernelGGL((k_perm_rank<kPermBlock, kPermItems, false>), dim3(tiles), dim3(kPermBlock), 0, s,
                           (const uint64_t*)sorted, d_sa, n, toff, p.s1, 0u, cur1, other);
    const uint64_t* placed = other;
    if (p.s1 > p.s2) {
        if ((((uint32_t)c->tune >> 24) & 0xFu) == 1u) {   // A/B: the persistent prefetching split
            uint32_t* tk = perm_tickets(c);
            SA_HIP(hipMemsetAsync(tk, 0, 8 * 4, s));
            hipLaunchKernelGGL((k_split_p<kPermBlock, kPermItems>), dim3(2 * (uint32_t)c->cus), dim3(kPermBlock), 0, s,
                               (const uint64_t*)other, n, p.s1, p.s2, p.nb1, 1u, (uint64_t)0, p.tpb,
                               (const uint32_t*)nullptr, 0u, cur2, sorted, tk);
        } else {
            hipLaunchKernelGGL((k_perm_split<kPermBlock, kPermItems>), dim3((p.nb1 + 7) / 8 * 8 * p.tpb),
                               dim3(kPermBlock), 0, s, (const uint64_t*)other, n, p.s1, p.s2, p.tpb, cur2, sorted);
        }
        placed = sorted;
    }
    if (nh.out) {   // the next round's first-digit counts too (persistent: one count flush per workgroup)
        SA_HIP(hipMemsetAsync(nh.out, 0, 8 * kLsdMaxRadix * 4, s));
        const uint64_t nsub = (n + (1ull << kPermSub) - 1) >> kPermSub;
        const uint64_t g = std::min<uint64_t>(nsub, 2ull * (uint64_t)c->cus);   // two workgroups per CU
        const uint32_t spb = (uint32_t)((nsub + g - 1) / g);
        hipLaunchKernelGGL((k_perm_place<kPermBlock, true>), dim3((uint32_t)((nsub + spb - 1) / spb)),
                           dim3(kPermBlock), 0, s, placed, n, c->rank, c->words + kPermErrWord, nh, spb);
    } else {
        hipLaunchKernelGGL((k_perm_place<kPermBlock>), dim3((uint32_t)((n + (1ull << kPermSub) - 1) >> kPermSub)),
                           dim3(kPermBlock), 0, s, placed, n, c->rank, c->words + kPermErrWord);
    }
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_RERANK, (p.s1 > p.s2 ? 48ull : 32ull) * n - (kshift ? 4ull * n : 0ull));
    return SA_OK;
}

// ---------------------------------------------------------------------------
// the reference schedule's LSD sort (sa_lsd.h)
// ---------------------------------------------------------------------------
static uint32_t* lsd_ghist(sa_context* c) { return c->lsd; }
static uint32_t* lsd_base(sa_context* c) { return c->lsd + kMaxPasses * kLsdMaxRadix; }
static uint32_t* lsd_tickets(sa_context* c) { return c->lsd + 2 * kMaxPasses * kLsdMaxRadix; }

// widest digit of the plan (sa_opts.tune bits 0-7 = 8 restores 8-bit
// digits, A/B)
static uint32_t lsd_max_bits(const sa_context* c) {
    const uint32_t b = (uint32_t)c->tune & 0xFFu;
    return b ? std::min<uint32_t>(10, std::max<uint32_t>(8, b)) : 10u;
}

// B key bits above bit `base`: the pass count and widths of least relative
// cost, a pass of 9 / 10 bits costing ~1.2 / 1.45 of an 8-bit one (longer
// match-any, shorter digit runs per tile)
static LsdPlan lsd_plan(uint32_t B, uint32_t base, uint32_t maxb) {
    auto cost = [](uint32_t w) { return w <= 8 ? 1.0 : w == 9 ? 1.2 : 1.45; };
    LsdPlan pl{};
    double best = 1e30;
    for (uint32_t p = std::max<uint32_t>(1, (B + maxb - 1) / maxb); p <= std::max<uint32_t>(1, (B + 7) / 8); ++p) {
        double cst = 0;
        for (uint32_t i = 0; i < p; ++i) cst += cost(B / p + (i < B % p ? 1u : 0u));
        if (cst < best - 1e-9) {
            best = cst;
            pl.P = p;
        }
    }
    uint32_t sh = base;
    for (uint32_t i = 0; i < pl.P; ++i) {
        pl.bits[i] = std::max<uint32_t>(1, B / pl.P + (i < B % pl.P ? 1u : 0u));
        pl.shift[i] = sh;
        sh += pl.bits[i];
    }
    return pl;
}

// resident workgroups per CU of a persistent kernel (a property of the code
// object, the same on every gfx950 device; the grid is this times the
// launching context's CU count)
template <class K>
static int blocks_per_cu(K kernel, int block) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0) != hipSuccess || nb < 1) nb = 1;
    return nb;
}

// XQ (sa_lsd.h): per-XCD queues of tiles; base = qbase[8][1024], ticket =
// the pass's 8 queue tickets, next_hist = the next pass's per-queue counts;
// the grid is whole XCDs (every queue served)
// where a pass finds its digit bases and ticket(s) and writes its pairs; the
// next pass's digit, counted by this one into next_hist (null: the last pass)
struct LsdIo {
    const uint32_t* base;
    uint32_t* ticket;
    uint64_t* ok;
    uint32_t* ov;
    uint32_t nshift, nnbits;
    uint32_t* next_hist;
    QDiv qd;
    uint32_t tpq;
};
template <class Src, bool PACKED, bool XQ = false>
static int lsd_pass(Run& r, const Src& src, uint64_t n, uint32_t shift, uint32_t nbits, const LsdIo& io) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    const uint32_t epoch = next_epoch(c, s);
    uint64_t tiles = 0;
    unsigned long long* prof = reinterpret_cast<unsigned long long*>(lsd_tickets(c) + kMaxPasses);
    if (SA_LSD_PROF) hipMemsetAsync(prof, 0, 5 * 8, s);
#define SA_LSD_LAUNCH(RB)                                                                                   \
    do {                                                                                                    \
        auto kern = k_lsd<Src, RB, PACKED, XQ>;                                                             \
        constexpr int B = lsd_block<PACKED, RB, XQ>();                                                      \
        constexpr uint64_t T = (uint64_t)B * lsd_items<PACKED, RB, XQ>();                                   \
        tiles = (n + T - 1) / T;                                                                            \
        static std::atomic<int> per_cu{0};                                                                  \
        if (!per_cu.load(std::memory_order_relaxed)) per_cu.store(blocks_per_cu(kern, B));                  \
        const uint64_t grid = (uint64_t)c->cus * (uint64_t)per_cu.load(std::memory_order_relaxed);          \
        hipLaunchKernelGGL(kern, dim3((uint32_t)(XQ ? grid : std::min<uint64_t>(tiles, grid))), dim3(B), 0, s, \
                           src, n, shift, nbits, io.base, c->states, io.ticket, epoch, io.ok, io.ov,             \
                           c->words + kLookbackWord, prof, io.nshift, io.nnbits, io.next_hist, io.qd, io.tpq);   \
    } while (0)
    if (nbits <= 8) SA_LSD_LAUNCH(8);
    else if (nbits == 9) SA_LSD_LAUNCH(9);
    else if constexpr (PACKED || !XQ) SA_LSD_LAUNCH(10);
    else   // unpacked XQ passes take <= 9 bits (lsd_xq_ok): a wider one would write nothing
        return set_err(SA_E_INTERNAL, "unpacked per-XCD LSD pass of %u bits", nbits);
#undef SA_LSD_LAUNCH
    if (SA_LSD_PROF) {
        unsigned long long h[5];
        hipMemcpyAsync(h, prof, sizeof h, hipMemcpyDeviceToHost, s);
        host_sync(s);
        double tot = 0;
        for (double x : h) tot += x;
        std::fprintf(stderr, "[lsd-prof] n=%llu bits=%u packed=%d clk/tile %.0f: rank %.1f%% scan %.1f%% lookback %.1f%% stage %.1f%% write %.1f%%\n",
                     (unsigned long long)n, nbits, (int)PACKED, tot / (double)tiles,
                     100 * h[0] / tot, 100 * h[1] / tot, 100 * h[2] / tot, 100 * h[3] / tot, 100 * h[4] / tot);
    }
    return SA_OK;
}

// per-XCD queues of 8192-pair tiles (sa_lsd.h XQ): whether a sort takes
// them (unpacked passes of 10 bits do not fit their LDS with the per-queue
// counters) and the queue span
static bool lsd_xq_ok(const sa_context* c, uint64_t n, const LsdPlan& pl, bool packed) {
    const uint64_t xtiles = (n + kLsdXqTile - 1) / kLsdXqTile;
    bool xq = SA_LSD_XQ && c->cus % 8 == 0 && xtiles >= 64 && !(c->dbg & SA_DEBUG_NO_XQ);
    if (!packed)
        for (uint32_t p = 0; p < pl.P; ++p) xq = xq && pl.bits[p] <= 9;
    return xq;
}
// the span of a queue (qspan pairs = tpq tiles) and its divider, in the
// NextHist the re-rank takes them in
static NextHist lsd_xq_span(uint64_t n) {
    const uint64_t xtiles = (n + kLsdXqTile - 1) / kLsdXqTile;
    NextHist x;
    x.qspan = (xtiles + 7) / 8 * kLsdXqTile;
    x.qd.magic = (uint64_t)((((unsigned __int128)1 << 64) + x.qspan - 1) / x.qspan);
    return x;
}

// Stable LSD sort of n pairs by the plan's digits, pass 0 reading `first`.
// PACKED: one item buffer ping-pong; else keys + values, the last pass
// writing its values into vals_final.  sorted->keys: the sorted key / item buffer.
// hist_ready (XQ): the first pass's per-queue counts are already in
// lsdx[0] (the previous round's k_perm_place counted them).
template <bool PACKED, class Src0>
static int lsd_sort(Run& r, const Src0& first, uint64_t n, const LsdPlan& pl, uint32_t* vals_final,
                    uint32_t* vals_other, Sorted* sorted, bool hist_ready = false) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    if (pl.P < 1 || pl.P > kMaxPasses) return set_err(SA_E_INTERNAL, "%u radix passes", pl.P);
    uint64_t* kb[2] = {c->keys[0], c->keys[1]};
    uint32_t* vb[2];
    vb[(pl.P - 1) & 1] = vals_final;
    vb[pl.P & 1] = vals_other;
    SA_HIP(hipMemsetAsync(c->lsd, 0, (2 * kMaxPasses * kLsdMaxRadix + kMaxPasses) * 4, s));
    // the first digit's totals here; every pass counts the next one's
    LsdPlan first_only = pl;
    first_only.P = 1;
    const uint64_t pair = PACKED ? 8 : 12;
    const dim3 hgrid((uint32_t)std::min<uint64_t>((n + 8 * kBlock - 1) / (8 * kBlock), (uint64_t)c->cus * 4));
    // pass p from its source (pass 0: `first`) into the other buffers
    auto pass = [&](auto xq, uint32_t p, const LsdIo& io) -> int {
        constexpr bool XQ = decltype(xq)::value;
        r.begin(p == 0 ? SA_K_SCATTER_FIRST : SA_K_SCATTER_KEYS);
        if (p == 0)
            SA_TRY(lsd_pass<Src0, PACKED, XQ>(r, first, n, pl.shift[0], pl.bits[0], io));
        else if constexpr (PACKED)
            SA_TRY(lsd_pass<SrcItems, true, XQ>(r, SrcItems{kb[(p - 1) & 1]}, n, pl.shift[p], pl.bits[p], io));
        else
            SA_TRY(lsd_pass<SrcKeys, false, XQ>(r, SrcKeys{kb[(p - 1) & 1], vb[(p - 1) & 1]}, n, pl.shift[p],
                                                pl.bits[p], io));
        r.end();
        r.bytes(p == 0 ? SA_K_SCATTER_FIRST : SA_K_SCATTER_KEYS, (p == 0 ? 8 + pair : 2 * pair) * n);
        return SA_OK;
    };
    // per-XCD queues of tiles (sa_lsd.h XQ): counts [pass][8][1024], bases [8][1024], tickets [pass][8 x 32]
    const bool xq = lsd_xq_ok(c, n, pl, PACKED);
    const NextHist x = xq ? lsd_xq_span(n) : NextHist{};
    uint32_t* const qh = c->lsdx;
    uint32_t* const qb = qh + kMaxPasses * 8 * kLsdMaxRadix;
    uint32_t* const qt = qb + 8 * kLsdMaxRadix;
    if (xq && hist_ready) {   // pass 0's counts came with the previous round's re-rank
        SA_HIP(hipMemsetAsync(c->lsdx + 8 * kLsdMaxRadix, 0, (kLsdXqWords - 8 * kLsdMaxRadix) * 4, s));
    } else {
        if (xq) SA_HIP(hipMemsetAsync(c->lsdx, 0, kLsdXqWords * 4, s));
        r.begin(SA_K_HIST_FIRST);
        if (xq) hipLaunchKernelGGL(k_lsd_hist<Src0>, hgrid, dim3(kBlock), 0, s, first, n, first_only, qh, x.qd);
        else hipLaunchKernelGGL(k_lsd_hist<Src0>, hgrid, dim3(kBlock), 0, s, first, n, first_only, lsd_ghist(c));
        r.end();
        r.bytes(SA_K_HIST_FIRST, 8 * n);
    }
    for (uint32_t p = 0; p < pl.P; ++p) {
        uint32_t* const base = xq ? qb : lsd_base(c) + p * kLsdMaxRadix;
        r.begin(SA_K_SCAN);
        if (xq)
            hipLaunchKernelGGL(k_lsd_qbase, dim3(1), dim3(1024), 0, s, (const uint32_t*)qh + p * 8 * kLsdMaxRadix,
                               1u << pl.bits[p], qb);
        else
            hipLaunchKernelGGL(k_digit_base_wide, dim3(1), dim3(1024), 0, s,
                               (const uint32_t*)lsd_ghist(c) + p * kLsdMaxRadix, 1u << pl.bits[p], base);
        r.end();
        const bool more = p + 1 < pl.P;
        uint32_t* const counts = xq ? qh + (p + 1) * 8 * kLsdMaxRadix : lsd_ghist(c) + (p + 1) * kLsdMaxRadix;
        const LsdIo io{base, xq ? qt + p * 8 * 32 : lsd_tickets(c) + p, kb[p & 1], PACKED && p ? nullptr : vb[p & 1],
                       more ? pl.shift[p + 1] : 0u, more ? pl.bits[p + 1] : 1u, more ? counts : nullptr,
                       x.qd, (uint32_t)(x.qspan / kLsdXqTile)};
        if (xq) SA_TRY(pass(std::true_type{}, p, io));
        else SA_TRY(pass(std::false_type{}, p, io));
    }
    SA_HIP(hipGetLastError());
    *sorted = Sorted{kb[(pl.P - 1) & 1], pl.P};
    return SA_OK;
}

// the reference schedule: manber_myers.c:88-125 round for round
#include "sa_reference.h"

// the packed schedule: round 1 by K symbols, then doubling rounds over the
// unsorted set only
#include "sa_packed.h"

static int build_device(sa_context* c, const uint8_t* d_text, uint64_t n, uint32_t* d_sa, hipStream_t s,
                        const sa_opts* opts, sa_stats* st) {
    if (st) {
        std::memset(st, 0, sizeof *st);
        st->n_kinds = SA_K_COUNT;
    }
    const int schedule = opts ? opts->schedule : SA_SCHEDULE_PACKED;
    if (st) st->schedule = schedule;
    if (n == 0) return SA_OK;
    if (!d_text || !d_sa) return set_err(SA_E_INVALID, "NULL device pointer");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n = %llu exceeds 2^32-1 on one device",
                                          (unsigned long long)n);
    if (schedule != SA_SCHEDULE_PACKED && schedule != SA_SCHEDULE_REFERENCE)
        return set_err(SA_E_INVALID, "unknown schedule %d", schedule);
    SA_HIP(hipSetDevice(c->device));
    SA_TRY(ensure_capacity(c, n));
    Run r{c, s, opts && opts->profile, st};
    c->radix = opts ? opts->radix : 0;
    set_debug(c, opts);
    if (c->radix != 0 && c->radix != 1) return set_err(SA_E_INVALID, "unknown radix algorithm %d", c->radix);
    SA_HIP(hipMemsetAsync(c->words, 0, 64, s));
    Events ev;
    SA_TRY(ev.make());
    SA_TRACE("build n=%llu schedule=%d", (unsigned long long)n, schedule);
    SA_HIP(hipEventRecord(ev.e[0], s));
    if (n == 1) {
        SA_HIP(hipMemsetAsync(d_sa, 0, 4, s));
    } else if (schedule == SA_SCHEDULE_REFERENCE) {
        SA_TRY(build_reference(r, d_text, n, d_sa));
    } else {
        SA_TRY(build_packed(r, d_text, n, d_sa, opts));
    }
    SA_HIP(hipEventRecord(ev.e[1], s));
    SA_HIP(hipEventSynchronize(ev.e[1]));
    r.flush();
    r.round_times();
    if (st) st->total_ms = elapsed(ev.e[0], ev.e[1]);
    return SA_OK;
}

#include "sa_dist.h"

// ---------------------------------------------------------------------------
// O(n) checker (replaces is_valid_suffix_array, manber_myers.c:184-202)
// ---------------------------------------------------------------------------

// level-1 stripes of a permutation (sa_check.h BinStripes): `want` per bin
// when keys[0] holds the regions with their slack (2^s1 / 128, >= 2048:
// ~45 standard deviations of a stripe's fill at 1 GiB), else one
static BinStripes plan_stripes(const sa_context* c, uint64_t n, const PermPlan& p, uint32_t want) {
    BinStripes bs;
    if (want <= 1 || n < (1ull << 24)) return bs;
    const uint64_t per = ((1ull << p.s1) + want - 1) / want;
    const uint64_t scap = per + std::max<uint64_t>(2048, (1ull << p.s1) / 128);
    if ((uint64_t)p.nb1 * want * scap > c->cap_pad) return bs;
    bs.st = want;
    bs.scap = scap;
    return bs;
}

constexpr uint32_t kChkStripes = 8;   // one per XCD
constexpr uint32_t kCur2 = 1024 * kChkStripes;   // hist: level-1 cursors [stripe][bin], then level 2's

// the checker's level-1 bin bits (sa_check.h k_chk_bin NB): 8 by default;
// sa_context_set_debug's tune bits 20-23 = 1 / 2 select 10 / 9 (A/B runs)
// the checker's level-2 kernel: tune bits 20-23 = 3 take the persistent
// prefetching k_split_p (A/B runs)
static bool chk_split_persistent(const sa_context* c) { return (((uint32_t)c->tune >> 20) & 0xFu) == 3u; }

static uint32_t chk_stride(const PermPlan& p) { return p.nb1 <= 256 ? 256u : p.nb1 <= 512 ? 512u : 1024u; }

static uint32_t chk_bin_bits(const sa_context* c) {
    const uint32_t v = ((uint32_t)c->tune >> 20) & 0xFu;
    return v == 1 ? 10u : v == 2 ? 9u : 8u;
}

// Levels 1 and 2 of a permutation: (dest, value) pairs of `src` binned by
// dest (level-1 cursors per stripe and bin) and split into 2^s2-entry
// sub-bins of the final layout (keys[1], or keys[0] when s1 == s2); returns
// the pairs' buffer.  Cursors in hist (zeroed here).
template <class Src, int DSH, int TAG>
static const uint64_t* permute_levels(sa_context* c, const Src& src, uint64_t n, const PermPlan& p,
                                      const BinStripes& bs, uint32_t* err, hipStream_t s, int* rc) {
    *rc = SA_OK;
    if (hipMemsetAsync(c->hist, 0, ((uint64_t)kCur2 + (uint64_t)p.nb1 * p.nsub) * 4, s) != hipSuccess) {
        *rc = set_err(SA_E_HIP, "hipMemsetAsync failed");
        return nullptr;
    }
    const uint32_t fstride = chk_stride(p);   // cursors per stripe: k_chk_bin's NB
    if (fstride == 256) {
        constexpr uint64_t T = (uint64_t)kChkBlock * kChkItems;
        hipLaunchKernelGGL((k_chk_bin<kChkBlock, kChkItems, Src, 256>), dim3((uint32_t)((n + T - 1) / T)),
                           dim3(kChkBlock), 0, s, src, n, p.s1, c->hist, c->keys[0], err, bs);
    } else if (fstride == 512) {   // 16-bit bin tags: 7 items per lane keep two workgroups per CU
        constexpr uint64_t T = (uint64_t)kChkBlock * 7;
        hipLaunchKernelGGL((k_chk_bin<kChkBlock, 7, Src, 512>), dim3((uint32_t)((n + T - 1) / T)), dim3(kChkBlock),
                           0, s, src, n, p.s1, c->hist, c->keys[0], err, bs);
    } else {
        constexpr uint64_t T = (uint64_t)kChkBlock * 7;
        hipLaunchKernelGGL((k_chk_bin<kChkBlock, 7, Src, 1024>), dim3((uint32_t)((n + T - 1) / T)), dim3(kChkBlock),
                           0, s, src, n, p.s1, c->hist, c->keys[0], err, bs);
    }
    if (p.s1 == p.s2 && bs.st == 1) return c->keys[0];
    if (chk_split_persistent(c)) {
        uint32_t* tk = perm_tickets(c);
        if (hipMemsetAsync(tk, 0, 8 * 4, s) != hipSuccess) {
            *rc = set_err(SA_E_HIP, "hipMemsetAsync failed");
            return nullptr;
        }
        const uint32_t tpr = bs.st > 1 ? (uint32_t)((bs.scap + kPermBlock * kPermItems - 1) / (kPermBlock * kPermItems))
                                       : p.tpb;
        hipLaunchKernelGGL((k_split_p<kPermBlock, kPermItems, DSH, true, TAG>), dim3(2 * (uint32_t)c->cus),
                           dim3(kPermBlock), 0, s, (const uint64_t*)c->keys[0], n, p.s1, p.s2, p.nb1, bs.st, bs.scap,
                           tpr, (const uint32_t*)c->hist, fstride, c->hist + kCur2, c->keys[1], tk);
        return c->keys[1];
    }
    if (bs.st > 1) {
        const uint32_t tps = (uint32_t)((bs.scap + kPermBlock * kPermItems - 1) / (kPermBlock * kPermItems));
        hipLaunchKernelGGL((k_chk_split<kPermBlock, kPermItems, DSH, TAG>), dim3((p.nb1 + 7) / 8 * 8 * bs.st * tps),
                           dim3(kPermBlock), 0, s, (const uint64_t*)c->keys[0], n, p.s1, p.s2, bs, tps,
                           (const uint32_t*)c->hist, fstride, c->hist + kCur2, c->keys[1]);
    } else {
        hipLaunchKernelGGL((k_perm_split<kPermBlock, kPermItems, DSH, true, TAG>), dim3((p.nb1 + 7) / 8 * 8 * p.tpb),
                           dim3(kPermBlock), 0, s, (const uint64_t*)c->keys[0], n, p.s1, p.s2, p.tpb,
                           c->hist + kCur2, c->keys[1]);
    }
    return c->keys[1];
}

// (dest, value) pairs of `src` placed by dest into out[0, n) by the
// coalesced permutation: LCP's PHI.  Holes (0) and misplaced pairs set bits
// of *err; *err bit 128: a stripe overflowed (the caller runs it again with
// stripes = 1).  SUB: k_perm_place's (what is written is the value - SUB).
template <class Src, int TAG, uint32_t SUB = 0>
static int place_by_permutation(sa_context* c, const Src& src, uint64_t n, uint32_t* out, uint32_t* err,
                                hipStream_t s, uint32_t stripes) {
    const PermPlan p = plan_check(n, kChkSubA);
    if (p.nb1 > 256 || p.nsub > kPermMaxSub || p.s1 > 24)
        return set_err(SA_E_INTERNAL, "permutation plan out of range (n=%llu)", (unsigned long long)n);
    int rc = SA_OK;
    const uint64_t* placed = permute_levels<Src, 32, TAG>(c, src, n, p, plan_stripes(c, n, p, stripes), err, s, &rc);
    if (rc) return rc;
    hipLaunchKernelGGL((k_perm_place<kPermBlock, false, TAG, SUB>), dim3((uint32_t)((n + (1ull << kPermSub) - 1) >> kPermSub)),
                       dim3(kPermBlock), 0, s, placed, n, out, err);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// the stripes place_by_permutation runs with when `stripes` are asked for
// (SA_TRACE: a context too small for the regions runs one)
static uint32_t perm_stripes_run(const sa_context* c, uint64_t n, uint32_t stripes) {
    return plan_stripes(c, n, plan_check(n, kChkSubA), stripes).st;
}

// sa_check.h: pass A (ISA' by permutation) and pass B (adjacent keys compared
// in LDS per sorted sub-bin); one host sync at the end.  Workspace: ISA' in
// rank, pairs in keys[0] / keys[1], cursors in hist, sub-bin end keys in
// vals_alt.  Returns 1 valid, 0 invalid, < 0 an error.
static int check_device(sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, hipStream_t s) {
    if (n == 0) return 1;
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (!d_text || !d_sa) return set_err(SA_E_INVALID, "NULL device pointer");
    SA_HIP(hipSetDevice(c->device));
    int rc = ensure_capacity(c, n);
    if (rc) return rc;
    uint32_t* isa = c->rank;
    uint32_t* err = c->words + kChkErrWord;
    uint32_t* cur1 = c->hist;
    uint32_t* cur2 = c->hist + kCur2;
    uint64_t* ends = reinterpret_cast<uint64_t*>(c->vals_alt);
    uint32_t bits = 0;   // the error bits of the last run
    for (uint32_t stripes : {kChkStripes, 1u}) {
        SA_HIP(hipMemsetAsync(err, 0, 4, s));
        uint32_t ran[2] = {1, 1};   // the stripes plan_stripes granted (SA_TRACE)
        for (int pass = 0; pass < 2; ++pass) {
            // pass B's sub-bins: 2^13, or 2^14 once a bin would split into more
            // than the split pass's kPermMaxSub (n > 2^31)
            const uint32_t lg = bit_width(n > 1 ? n - 1 : 1);
            const uint32_t s2b = (lg > 8 && lg - 8 > kChkSubB + 10) ? kChkSubB + 1 : kChkSubB;
            const PermPlan p = plan_check(n, pass ? s2b : kChkSubA, chk_bin_bits(c));
            if (p.nb1 > 1024 || p.nsub > kPermMaxSub || p.s1 > 24)
                return set_err(SA_E_INTERNAL, "checker plan out of range (n=%llu)", (unsigned long long)n);
            const BinStripes bs = plan_stripes(c, n, p, stripes);
            ran[pass] = bs.st;
            const uint64_t* placed =
                pass == 0 ? permute_levels<ChkSrcA, 32, 1>(c, ChkSrcA{d_sa}, n, p, bs, err, s, &rc)
                          : permute_levels<ChkSrcB, 40, 1>(c, ChkSrcB{isa, d_text}, n, p, bs, err, s, &rc);
            if (rc) return rc;
            hipLaunchKernelGGL(k_chk_cursors,
                               dim3((uint32_t)std::min<uint64_t>(((uint64_t)p.nb1 * (p.nsub + 1) + kBlock - 1) / kBlock, 1024)),
                               dim3(kBlock), 0, s, (const uint32_t*)cur1, (const uint32_t*)cur2, n, p.s1, p.s2, p.nb1,
                               err, bs.st, chk_stride(p));
            const uint64_t nsb = (n + (1ull << p.s2) - 1) >> p.s2;
            if (pass == 0) {
                hipLaunchKernelGGL((k_perm_place<kPermBlock, false, 1>), dim3((uint32_t)nsb), dim3(kPermBlock), 0, s,
                                   placed, n, isa, err);
            } else {
                if (p.s2 == kChkSubB)
                    hipLaunchKernelGGL((k_chk_place<kChkBlock>), dim3((uint32_t)nsb), dim3(kChkBlock), 0, s, placed, n,
                                       p.s1, ends, err);
                else
                    hipLaunchKernelGGL((k_chk_place<kChkBlock, kChkSubB + 1>), dim3((uint32_t)nsb), dim3(kChkBlock), 0,
                                       s, placed, n, p.s1, ends, err);
                hipLaunchKernelGGL(k_chk_tiles, dim3((uint32_t)std::min<uint64_t>((nsb + kBlock - 1) / kBlock, 1024)),
                                   dim3(kBlock), 0, s, (const uint64_t*)ends, nsb, err);
            }
        }
        SA_HIP(hipGetLastError());
        SA_READ(w, read_word(c, kChkErrWord, s));
        bits = *w;
        SA_TRACE("check (%u stripes asked, %u / %u run in pass A / B): error bits %#x", stripes, ran[0], ran[1], bits);
        if (!(bits & 128u)) break;   // else a stripe overflowed: again with one
    }
    return bits == 0 ? 1 : 0;
}

// place_by_permutation with kChkStripes stripes and, when one of them overflowed
// (only an adversarial SA: it lost pairs), again with one; the error bits stay in
// words[kPlaceErrWord].  (drop the wait when one stripe was granted.)
template <class Src, int TAG>
static int place_striped(sa_context* c, const Src& src, uint64_t n, uint32_t* out, hipStream_t s, const char* what) {
    for (uint32_t stripes : {kChkStripes, 1u}) {
        SA_HIP(hipMemsetAsync(c->words + kPlaceErrWord, 0, 4, s));
        SA_TRY(place_by_permutation<Src, TAG>(c, src, n, out, c->words + kPlaceErrWord, s, stripes));
        if (stripes == 1) {
            SA_TRACE("lcp %s (%u stripes asked, %u run)", what, stripes, perm_stripes_run(c, n, stripes));
            break;
        }
        SA_READ(bits, read_word(c, kPlaceErrWord, s));
        SA_TRACE("lcp %s (%u stripes asked, %u run): error bits %#x", what, stripes, perm_stripes_run(c, n, stripes),
                 *bits);
        if (!(*bits & 128u)) break;
    }
    return SA_OK;
}

// ---------------------------------------------------------------------------
// LCP + LRS (sa_lcp.h).  Workspace: PHI lives in d_lcp until the gather
// overwrites it, v / PLCP in rank, the cooperative pair lists in keys[0..1],
// their first-mismatch words in vals_alt, pair counts in counts, chunk maxima
// in hist, the LRS key in words[8..9].
// ---------------------------------------------------------------------------
// the longest repeated substring: its length and one position (0, 0: none)
struct Lrs {
    uint64_t len = 0, pos = 0;
};
static int lcp_device(sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint32_t* d_lcp,
                      Lrs* lrs, hipStream_t s) {
    if (lrs) *lrs = Lrs{};
    if (n == 0) return SA_OK;
    if (!d_text || !d_sa || !d_lcp) return set_err(SA_E_INVALID, "NULL device pointer");
    if ((const void*)d_sa == (const void*)d_lcp) return set_err(SA_E_INVALID, "d_lcp may not alias d_sa");
    // PHI and the final LCP are placed into d_lcp by k_perm_place, which stores uint4
    if ((uintptr_t)d_lcp & 15) return set_err(SA_E_INVALID, "d_lcp must be 16-byte aligned");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    SA_HIP(hipSetDevice(c->device));
    int rc = ensure_capacity(c, n);
    if (rc) return rc;
    uint32_t* phi = d_lcp;
    uint32_t* v = c->rank;
    uint32_t* cnt = c->counts;   // [k] = pairs in list k
    unsigned long long* best = reinterpret_cast<unsigned long long*>(c->words + 8);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, 16384);
    SA_HIP(hipMemsetAsync(cnt, 0, (kLongRounds + 1) * 4, s));
    SA_HIP(hipMemsetAsync(best, 0, 8, s));
    // PHI' = PHI + 1 (0: none) by the coalesced permutation (its hole flag for
    // the smallest suffix, which has no predecessor, is expected: words[12])
    SA_TRY(place_striped<PhiSrc, 2>(c, PhiSrc{d_sa}, n, phi, s, "PHI"));
    hipLaunchKernelGGL(k_plcp_irreducible, dim3(grid), dim3(kBlock), 0, s, d_text, n, (const uint32_t*)phi, v,
                       c->keys[0], c->vals_alt, cnt);
    uint64_t lo = kDirect;
    for (int k = 0; k < kLongRounds && lo < n; ++k, lo *= 4) {
        const uint64_t* list = c->keys[k & 1];
        uint64_t* next = c->keys[(k + 1) & 1];
        hipLaunchKernelGGL(k_plcp_long, dim3(4096), dim3(kBlock), 0, s, d_text, n, list,
                           (const uint32_t*)(cnt + k), lo, std::min<uint64_t>(4 * lo, n), c->vals_alt);
        hipLaunchKernelGGL(k_plcp_settle, dim3(1024), dim3(kBlock), 0, s, list, (const uint32_t*)(cnt + k),
                           c->vals_alt, v, next, cnt + k + 1);
    }
    const Chunking ch = plan_chunks(n);
    hipLaunchKernelGGL(k_chunk_max, dim3(ch.chunks), dim3(kBlock), 0, s, (const uint32_t*)v, ch, c->hist);
    hipLaunchKernelGGL(k_scan_chunk_max, dim3(1), dim3(kBlock), 0, s, c->hist, ch.chunks);
    hipLaunchKernelGGL(k_plcp_apply, dim3(ch.chunks), dim3(kBlock), 0, s, v, ch, (const uint32_t*)c->hist);
    // LCP[r] = PLCP[SA[r]] (:147-155): ISA + 1 by the coalesced permutation
    // (into vals_alt, free after the long rounds), then PLCP placed at ISA
    // -- 2 x ~8.6 ms of streamed traffic at 1 GiB against a 24.7 ms random
    // 4-byte gather (146 GB moved); tune bit 30: the gather (A/B runs)
    if ((((uint32_t)c->tune >> 30) & 1u) || n < 2) {
        hipLaunchKernelGGL(k_lcp_gather, dim3(grid), dim3(kBlock), 0, s, d_sa, n, (const uint32_t*)v, d_lcp, best);
    } else {
        uint32_t* isa1 = c->vals_alt;
        SA_TRY(place_striped<IsaSrc, 3>(c, IsaSrc{{d_sa}}, n, isa1, s, "ISA"));
        SA_TRY(place_striped<PlcpSrc, 4>(c, PlcpSrc{isa1, v}, n, d_lcp, s, "PLCP"));
        hipLaunchKernelGGL(k_lcp_best, dim3(grid), dim3(kBlock), 0, s, (const uint32_t*)d_lcp, n, best);
    }
    SA_HIP(hipGetLastError());
    SA_HIP(hipMemcpyAsync(c->host_words + hw(kHwLcpBest).at, best, 8, hipMemcpyDeviceToHost, s));
    SA_HIP(hipMemcpyAsync(c->host_words + hw(kHwLcpCounts).at, cnt, (kLongRounds + 1) * 4, hipMemcpyDeviceToHost, s));
    SA_HIP(host_sync(s));
    // every pair resolves by the last window (it reaches n); a pair left over is a bug
    uint64_t lo_end = kDirect;
    int rounds = 0;
    while (rounds < kLongRounds && lo_end < n) { lo_end *= 4; ++rounds; }
    const uint32_t* hl = c->host_words + hw(kHwLcpCounts).at;
    if (hl[rounds] != 0) return set_err(SA_E_INTERNAL, "%u LCP pairs unresolved", hl[rounds]);
    SA_TRACE("lcp: direct-overflow pairs %u, rounds %d", hl[0], rounds);
    unsigned long long b;
    std::memcpy(&b, c->host_words + hw(kHwLcpBest).at, 8);
    const uint64_t len = b >> 32;
    if (len) {
        const uint64_t r = 0xFFFFFFFFull - (b & 0xFFFFFFFFull);
        uint32_t pos = 0;
        SA_HIP(host_memcpy(&pos, d_sa + r, 4, hipMemcpyDeviceToHost));
        if (lrs) *lrs = Lrs{len, pos};
    }
    return SA_OK;
}

// ---------------------------------------------------------------------------
// seeded synthetic input on the device (SURVEY.md 8(d) splitmix64 spec), so
// benchmarks do not push gigabytes over PCIe
// ---------------------------------------------------------------------------
struct Alphabet {
    uint8_t sym[256];
};

__global__ __launch_bounds__(kBlock) void k_gen_text(uint8_t* __restrict__ out, uint64_t n, uint64_t seed,
                                                     Alphabet a, uint32_t sigma) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        out[i] = a.sym[((z >> 32) * (uint64_t)sigma) >> 32];
    }
}

}  // namespace sa

// the host side of the host-pointer entry points: staged copies, the
// process-wide context, device buffers freed by scope, and the host forms of
// sa_build_ex, sa_check and sa_lcp
#include "sa_host.h"

// batched pattern search (sa_find, sa_find_device): kernels, launches and its
// entry points
#include "sa_find.h"
// longest-match queries and matching statistics over the same search core
#include "sa_match.h"
// the Burrows-Wheeler transform and the inverse suffix array of a built SA
#include "sa_bwt.h"

using namespace sa;

extern "C" {

const char* sa_last_error(void) { return g_err.c_str(); }

uint64_t sa_host_syncs(void) { return g_host_syncs.load(std::memory_order_relaxed); }

const char* sa_version(void) { return "sa_hip gfx950 " __DATE__; }

int sa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

uint64_t sa_workspace_bytes(uint64_t max_n) { return ws_bytes(max_n); }

int sa_context_create(int device, uint64_t max_n, sa_context** out) {
    if (!out) return set_err(SA_E_INVALID, "out is NULL");
    *out = nullptr;
    int ndev = sa_device_count();
    if (ndev <= 0) return set_err(SA_E_HIP, "no HIP device visible (libsa_hip needs an MI355X)");
    if (device < 0 || device >= ndev) return set_err(SA_E_INVALID, "device %d out of range", device);
    SA_HIP(hipSetDevice(device));
    sa_context* c = new sa_context();
    c->device = device;
    if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->cus <= 0)
        c->cus = 256;
    if (hipMalloc(&c->hist, (size_t)kRadix * kMaxChunks * 4) != hipSuccess ||
        hipMalloc(&c->totals, kRadix * 4) != hipSuccess || hipMalloc(&c->counts, 4 * kMaxChunks * 4) != hipSuccess ||
        hipMalloc(&c->words, 64) != hipSuccess || hipMalloc(&c->alpha, 256 * 4) != hipSuccess ||
        hipMalloc(&c->code, 256 * 2) != hipSuccess ||
        hipMalloc(&c->os, (2 * kMaxPasses * kRadix + kMaxPasses) * 4) != hipSuccess ||
        hipMalloc(&c->lsd, (2 * kMaxPasses * kLsdMaxRadix + kMaxPasses) * 4 + 64) != hipSuccess ||
        hipMalloc(&c->lsdx, kLsdXqWords * 4) != hipSuccess ||
        hipMalloc(&c->segw, (kBstartOff + 2 * kBstartWords) * 4) != hipSuccess ||
        hipHostMalloc(&c->host_words, kHostWords * 4, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        sa_context_destroy(c);
        return set_err(SA_E_NOMEM, "context allocation failed");
    }
    for (int i = 0; i < kEvPool + kRoundEv + 1; ++i) {
        if (hipEventCreate(&c->ev[i]) != hipSuccess) {
            sa_context_destroy(c);
            return set_err(SA_E_HIP, "hipEventCreate failed");
        }
        c->ev_ready = i + 1;
    }
    if (max_n) {
        int rc = ensure_capacity(c, max_n);
        if (rc) {
            sa_context_destroy(c);
            return rc;
        }
    }
    *out = c;
    return SA_OK;
}

void sa_context_destroy(sa_context* c) {
    if (!c) return;
    hipSetDevice(c->device);
    free_dist(c);
    free_ctx_buffers(c);
    free_u_buffers(c);
    hipFree(c->alpha);
    hipFree(c->code);
    hipFree(c->os);
    hipFree(c->lsd);
    hipFree(c->lsdx);
    hipFree(c->segw);
    hipFree(c->segx);
    hipFree(c->hist);
    hipFree(c->totals);
    hipFree(c->counts);
    hipFree(c->words);
    if (c->host_words) hipHostFree(c->host_words);
    for (int i = 0; i < c->ev_ready; ++i) hipEventDestroy(c->ev[i]);
    delete c;
}

int sa_context_set_debug(sa_context* ctx, const sa_opts* opts) {
    if (!ctx) return set_err(SA_E_INVALID, "NULL context");
    set_debug(ctx, opts);
    return SA_OK;
}

int sa_build_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, uint32_t* d_sa, void* stream,
                    const sa_opts* opts, sa_stats* stats) {
    if (!ctx) return set_err(SA_E_INVALID, "context is NULL");
    const int rc = build_device(ctx, d_text, n, d_sa, (hipStream_t)stream, opts, stats);
    // this build's debug flags, span and launch shapes do not outlive it: a
    // later sa_dist_* build on the same context sees the defaults unless
    // sa_context_set_debug sets them again
    set_debug(ctx, nullptr);
    return rc;
}

int sa_check_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, void* stream) {
    if (!ctx) return set_err(SA_E_INVALID, "context is NULL");
    return check_device(ctx, d_text, n, d_sa, (hipStream_t)stream);
}

int sa_lcp_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint32_t* d_lcp,
                  uint64_t* lrs_len, uint64_t* lrs_pos, void* stream) {
    if (!ctx) return set_err(SA_E_INVALID, "context is NULL");
    Lrs lrs;
    const int rc = lcp_device(ctx, d_text, n, d_sa, d_lcp, &lrs, (hipStream_t)stream);
    if (lrs_len) *lrs_len = lrs.len;
    if (lrs_pos) *lrs_pos = lrs.pos;
    return rc;
}

int sa_lcp(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* lcp_out, uint64_t* lrs_len,
           uint64_t* lrs_pos) {
    return lcp_host(text, n, sa, sa_width, lcp_out, lrs_len, lrs_pos);
}

int sa_build_ex(const uint8_t* text, uint64_t n, void* sa_out, int sa_width, const sa_opts* opts,
                sa_stats* stats) {
    return build_host(text, n, sa_out, sa_width, opts, stats);
}

// dst[idx[i] - base] = src[i]; indices outside [base, base + dst_n) are
// skipped and counted (the host turns a non-zero count into an error).
__global__ __launch_bounds__(256) void k_scatter_u64(uint64_t* __restrict__ dst, uint64_t dst_n,
                                                     const int64_t* __restrict__ idx, int64_t base,
                                                     const uint64_t* __restrict__ src, uint64_t m,
                                                     unsigned long long* __restrict__ bad) {
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = (uint64_t)(idx[i] - base);
        if (j < dst_n) dst[j] = src[i];
        else ++nbad;
    }
    if (nbad) atomicAdd(bad, (unsigned long long)nbad);
}

int sa_scatter_u64_device(uint64_t* d_dst, uint64_t dst_n, const int64_t* d_idx, int64_t base,
                          const uint64_t* d_src, uint64_t m, void* stream) {
    if (m == 0) return SA_OK;
    if (!d_dst || !d_idx || !d_src) return set_err(SA_E_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* d_bad = nullptr;
    unsigned long long bad = 0;
    SA_HIP(hipMallocAsync((void**)&d_bad, 8, s));
    SA_HIP(hipMemsetAsync(d_bad, 0, 8, s));
    const uint32_t grid = (uint32_t)std::min<uint64_t>((m + 255) / 256, 8192);
    hipLaunchKernelGGL(k_scatter_u64, dim3(grid), dim3(256), 0, s, d_dst, dst_n, d_idx, base, d_src, m, d_bad);
    SA_HIP(hipGetLastError());
    SA_HIP(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, s));
    SA_HIP(hipFreeAsync(d_bad, s));
    SA_HIP(host_sync(s));
    if (bad) return set_err(SA_E_INVALID, "%llu scatter indices outside [%lld, %lld)", bad, (long long)base,
                            (long long)(base + (int64_t)dst_n));
    return SA_OK;
}

// dst[i] = src[idx[i] - base]; out-of-range indices write 0 and are counted.
__global__ __launch_bounds__(256) void k_gather_u64(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src,
                                                    uint64_t src_n, const int64_t* __restrict__ idx, int64_t base,
                                                    uint64_t m, unsigned long long* __restrict__ bad) {
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = (uint64_t)(idx[i] - base);
        uint64_t v = 0;
        if (j < src_n) v = src[j];
        else ++nbad;
        dst[i] = v;
    }
    if (nbad) atomicAdd(bad, (unsigned long long)nbad);
}

int sa_gather_u64_device(uint64_t* d_dst, const uint64_t* d_src, uint64_t src_n, const int64_t* d_idx, int64_t base,
                         uint64_t m, void* stream) {
    if (m == 0) return SA_OK;
    if (!d_dst || !d_idx || !d_src) return set_err(SA_E_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* d_bad = nullptr;
    unsigned long long bad = 0;
    SA_HIP(hipMallocAsync((void**)&d_bad, 8, s));
    SA_HIP(hipMemsetAsync(d_bad, 0, 8, s));
    const uint32_t grid = (uint32_t)std::min<uint64_t>((m + 255) / 256, 8192);
    hipLaunchKernelGGL(k_gather_u64, dim3(grid), dim3(256), 0, s, d_dst, d_src, src_n, d_idx, base, m, d_bad);
    SA_HIP(hipGetLastError());
    SA_HIP(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, s));
    SA_HIP(hipFreeAsync(d_bad, s));
    SA_HIP(host_sync(s));
    if (bad) return set_err(SA_E_INVALID, "%llu gather indices outside [%lld, %lld)", bad, (long long)base,
                            (long long)(base + (int64_t)src_n));
    return SA_OK;
}

}  // extern "C"

// Inclusive scans of m int64 values in place (running max: the group-start
// carries of the sample-sort driver; sum: its dense group ids): per-tile
// totals (256 lanes x 16 contiguous values), one workgroup scans the tile
// totals, each tile then scans itself from its carry.
constexpr int kRmBlock = 256, kRmItems = 16, kRmTile = kRmBlock * kRmItems;

struct ScanMax {
    static __device__ __forceinline__ int64_t id() { return INT64_MIN; }
    static __device__ __forceinline__ int64_t f(int64_t a, int64_t b) { return a > b ? a : b; }
};
struct ScanSum {
    static __device__ __forceinline__ int64_t id() { return 0; }
    static __device__ __forceinline__ int64_t f(int64_t a, int64_t b) { return a + b; }
};

template <class Op>
__device__ inline int64_t rm_block_incl(int64_t v, int64_t* s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(v, o, 64);
        if (lane >= o) v = Op::f(y, v);
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    int64_t c = Op::id();
    for (int q = 0; q < w; ++q) c = Op::f(c, s_w[q]);
    return Op::f(c, v);
}

// exclusive block scan: the inclusive value of the previous lane
template <class Op>
__device__ inline int64_t rm_block_excl(int64_t v, int64_t* s_w) {
    const int64_t incl = rm_block_incl<Op>(v, s_w);
    int64_t c = __shfl_up(incl, 1, 64);
    if ((threadIdx.x & 63) == 0) {
        c = Op::id();
        for (int q = 0; q < (int)(threadIdx.x >> 6); ++q) c = Op::f(c, s_w[q]);
    }
    return c;
}

template <class Op>
__global__ __launch_bounds__(kRmBlock) void k_rmax_tiles(const int64_t* __restrict__ v, uint64_t m,
                                                         int64_t* __restrict__ tmax) {
    __shared__ int64_t s_w[kRmBlock / 64];
    const uint64_t b0 = (uint64_t)blockIdx.x * kRmTile + (uint64_t)threadIdx.x * kRmItems;
    int64_t x = Op::id();
    for (int j = 0; j < kRmItems; ++j)
        if (b0 + j < m) x = Op::f(x, v[b0 + j]);
    x = rm_block_incl<Op>(x, s_w);
    if (threadIdx.x == kRmBlock - 1) tmax[blockIdx.x] = x;
}

// exclusive scan of the tile totals (one workgroup of kRmBlock lanes); the
// grand total lands in tmax[tiles]
template <class Op>
__global__ __launch_bounds__(kRmBlock) void k_rmax_carry(int64_t* __restrict__ tmax, uint64_t tiles) {
    __shared__ int64_t s_w[kRmBlock / 64];
    const uint64_t per = (tiles + kRmBlock - 1) / kRmBlock;
    const uint64_t a = (uint64_t)threadIdx.x * per, e = a + per < tiles ? a + per : tiles;
    int64_t x = Op::id();
    for (uint64_t i = a; i < e; ++i) x = Op::f(x, tmax[i]);
    int64_t c = rm_block_excl<Op>(x, s_w);
    for (uint64_t i = a; i < e; ++i) {
        const int64_t y = tmax[i];
        tmax[i] = c;
        c = Op::f(c, y);
    }
    if (a < tiles && e == tiles) tmax[tiles] = c;
}

template <class Op>
__global__ __launch_bounds__(kRmBlock) void k_rmax_apply(int64_t* __restrict__ v, uint64_t m,
                                                         const int64_t* __restrict__ tcarry) {
    __shared__ int64_t s_w[kRmBlock / 64];
    const uint64_t b0 = (uint64_t)blockIdx.x * kRmTile + (uint64_t)threadIdx.x * kRmItems;
    int64_t r[kRmItems];
    int64_t x = Op::id();
    for (int j = 0; j < kRmItems; ++j) {
        r[j] = b0 + j < m ? v[b0 + j] : Op::id();
        x = Op::f(x, r[j]);
    }
    int64_t c = Op::f(tcarry[blockIdx.x], rm_block_excl<Op>(x, s_w));
    for (int j = 0; j < kRmItems; ++j) {
        c = Op::f(c, r[j]);
        if (b0 + j < m) v[b0 + j] = c;
    }
}




// out[i] = #{ j : sorted[j] < q[i] } (<= with RIGHT): one lane per query
template <bool RIGHT>
__global__ __launch_bounds__(kBlock) void k_count_below(const uint64_t* __restrict__ sorted, uint64_t m,
                                                        const uint64_t* __restrict__ q, uint64_t nq,
                                                        int64_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t x = q[i];
        uint64_t lo = 0, hi = m;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (RIGHT ? sorted[mid] <= x : sorted[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        out[i] = (int64_t)lo;
    }
}


// Stream compaction of a byte mask: per-tile counts of the non-zero bytes
// (16 per lane), their exclusive sum (k_rmax_carry<ScanSum>), then each tile
// writes its positions in order.
__global__ __launch_bounds__(kRmBlock) void k_sel_count(const uint8_t* __restrict__ mask, uint64_t m,
                                                        int64_t* __restrict__ tcnt) {
    __shared__ int64_t s_w[kRmBlock / 64];
    const uint64_t b0 = (uint64_t)blockIdx.x * kRmTile + (uint64_t)threadIdx.x * kRmItems;
    int64_t c = 0;
    for (int j = 0; j < kRmItems; ++j) c += (b0 + j < m && mask[b0 + j]) ? 1 : 0;
    c = rm_block_incl<ScanSum>(c, s_w);
    if (threadIdx.x == kRmBlock - 1) tcnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(kRmBlock) void k_sel_write(const uint8_t* __restrict__ mask, uint64_t m,
                                                        const int64_t* __restrict__ toff, int64_t* __restrict__ out) {
    __shared__ int64_t s_w[kRmBlock / 64];
    const uint64_t b0 = (uint64_t)blockIdx.x * kRmTile + (uint64_t)threadIdx.x * kRmItems;
    uint32_t bits = 0;
    for (int j = 0; j < kRmItems; ++j) bits |= (b0 + j < m && mask[b0 + j]) ? 1u << j : 0u;
    int64_t o = toff[blockIdx.x] + rm_block_excl<ScanSum>((int64_t)__popc(bits), s_w);
    while (bits) {
        const int j = __builtin_ctz(bits);
        bits &= bits - 1u;
        out[o++] = (int64_t)(b0 + j);
    }
}

template <class Op>
static int scan_i64(int64_t* d_v, uint64_t m, hipStream_t s) {
    const uint64_t tiles = (m + kRmTile - 1) / kRmTile;
    if (tiles > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "m too large");
    int64_t* d_t = nullptr;
    SA_HIP(hipMallocAsync((void**)&d_t, (tiles + 1) * 8, s));
    hipLaunchKernelGGL(k_rmax_tiles<Op>, dim3((uint32_t)tiles), dim3(kRmBlock), 0, s, d_v, m, d_t);
    hipLaunchKernelGGL(k_rmax_carry<Op>, dim3(1), dim3(kRmBlock), 0, s, d_t, tiles);
    hipLaunchKernelGGL(k_rmax_apply<Op>, dim3((uint32_t)tiles), dim3(kRmBlock), 0, s, d_v, m, d_t);
    SA_HIP(hipGetLastError());
    SA_HIP(hipFreeAsync(d_t, s));
    return SA_OK;
}

// batched locate over a built SA: sorted hit lists in CSR form (its offsets
// are summed by scan_i64 above)
#include "sa_locate.h"

// what the queries below share: candidate tiles and lists, lists materialised then sorted
#include "sa_query.h"

// maximal exact matches of a query: seeds by sa_match.h, their hits by
// sa_locate.h, the left check, the right extension and the compaction here
#include "sa_mem.h"

// the longest previous factor array (nearest smaller values over the SA with
// LCP range minima) and the LZ77 factorisation parsed from it
#include "sa_lz.h"

// the repeats of the text as LCP intervals (right-maximal, maximal,
// supermaximal): nearest smaller values over the LCP array, sa_lz.h's walk
// with the comparison as a parameter
#include "sa_repeats.h"

// the LF-mapping of a BWT and the inverse transform (text and SA back from
// bwt and primary index): a counting sort by byte, then list ranking over
// hashed splitters
#include "sa_ibwt.h"

// an FM-index over (bwt, primary): rank blocks counted from the LF kernels'
// histogram, backward-search counting, locating through a sampled SA whose
// hit lists sa_query.h's ListSort sorts
#include "sa_fm.h"

// document collections over one suffix array: the document array and the
// previous-occurrence array (the context's radix sort), document frequency
// of SA intervals in one filtered pass, document listing whose ids
// sa_query.h's ListSort sorts
#include "sa_docs.h"

// longest common extensions: a range-minimum index over the LCP array (block
// minima, a sparse table inside each superblock and one over the
// superblocks), rank-interval minima, LCE of two positions and substring
// order, all by one query kernel
#include "sa_lce.h"

// k-mismatch pattern search: the pieces of the patterns by sa_find.h, their
// hits by sa_locate.h, a verify that also removes the duplicates over
// sa_query.h's tiles, the survivors sorted by its sort_lists
#include "sa_hamming.h"

// k-difference pattern search: sa_hamming.h's pieces as seeds, a banded
// bit-vector DP per candidate over sa_query.h's tiles, the ends sorted by its
// sort_lists and made unique, distances and starts by the DP run backwards
#include "sa_edit.h"

extern "C" {

int sa_running_max_i64_device(int64_t* d_v, uint64_t m, void* stream) {
    if (m == 0) return SA_OK;
    if (!d_v) return set_err(SA_E_INVALID, "NULL device pointer");
    return scan_i64<ScanMax>(d_v, m, (hipStream_t)stream);
}

int sa_inclusive_sum_i64_device(int64_t* d_v, uint64_t m, void* stream) {
    if (m == 0) return SA_OK;
    if (!d_v) return set_err(SA_E_INVALID, "NULL device pointer");
    return scan_i64<ScanSum>(d_v, m, (hipStream_t)stream);
}

int sa_count_below_u64_device(const uint64_t* d_sorted, uint64_t m, const uint64_t* d_q, uint64_t nq, int right,
                              int64_t* d_out, void* stream) {
    if (nq == 0) return SA_OK;
    if ((!d_sorted && m) || !d_q || !d_out) return set_err(SA_E_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nq + kBlock - 1) / kBlock, 8192);
    if (right) hipLaunchKernelGGL(k_count_below<true>, dim3(grid), dim3(kBlock), 0, s, d_sorted, m, d_q, nq, d_out);
    else hipLaunchKernelGGL(k_count_below<false>, dim3(grid), dim3(kBlock), 0, s, d_sorted, m, d_q, nq, d_out);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

int sa_select_u8_device(const uint8_t* d_mask, uint64_t m, int64_t* d_out, uint64_t* count, void* stream) {
    if (!count) return set_err(SA_E_INVALID, "count is NULL");
    *count = 0;
    if (m == 0) return SA_OK;
    if (!d_mask) return set_err(SA_E_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const uint64_t tiles = (m + kRmTile - 1) / kRmTile;
    if (tiles > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "m too large");
    int64_t* d_t = nullptr;
    int64_t total = 0;
    SA_HIP(hipMallocAsync((void**)&d_t, (tiles + 1) * 8, s));
    hipLaunchKernelGGL(k_sel_count, dim3((uint32_t)tiles), dim3(kRmBlock), 0, s, d_mask, m, d_t);
    hipLaunchKernelGGL(k_rmax_carry<ScanSum>, dim3(1), dim3(kRmBlock), 0, s, d_t, tiles);
    if (d_out) hipLaunchKernelGGL(k_sel_write, dim3((uint32_t)tiles), dim3(kRmBlock), 0, s, d_mask, m, d_t, d_out);
    SA_HIP(hipGetLastError());
    SA_HIP(hipMemcpyAsync(&total, d_t + tiles, 8, hipMemcpyDeviceToHost, s));
    SA_HIP(hipFreeAsync(d_t, s));
    SA_HIP(host_sync(s));
    *count = (uint64_t)total;
    return SA_OK;
}

int sa_alphabet_device(const uint8_t* d_text, uint64_t n, uint32_t present_out[8], void* stream) {
    if (!present_out) return set_err(SA_E_INVALID, "present_out is NULL");
    std::memset(present_out, 0, 32);
    if (n == 0) return SA_OK;
    if (!d_text) return set_err(SA_E_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* d_mask = nullptr;
    SA_HIP(hipMallocAsync((void**)&d_mask, 32, s));
    SA_HIP(hipMemsetAsync(d_mask, 0, 32, s));
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kBlock * 16 - 1) / (kBlock * 16), 2048);
    hipLaunchKernelGGL(k_alphabet, dim3(grid), dim3(kBlock), 0, s, d_text, n, d_mask);
    SA_HIP(hipGetLastError());
    SA_HIP(hipMemcpyAsync(present_out, d_mask, 32, hipMemcpyDeviceToHost, s));
    SA_HIP(hipFreeAsync(d_mask, s));
    SA_HIP(host_sync(s));
    return SA_OK;
}

int sa_pack_keys_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, uint64_t lo, uint64_t hi,
                        const uint16_t code[256], uint64_t base, uint32_t K, uint64_t* d_keys_out, void* stream) {
    if (lo > hi || hi > n) return set_err(SA_E_INVALID, "bad range [%llu, %llu) of %llu", (unsigned long long)lo,
                                          (unsigned long long)hi, (unsigned long long)n);
    if (K == 0 || K >= (uint32_t)kMaxK || base < 2 || key_bits(base, K) > 64)
        return set_err(SA_E_INVALID, "bad packing K=%u base=%llu", K, (unsigned long long)base);
    // an empty slice (n < world size) writes nothing: a zero-element tensor's
    // data pointer may be NULL
    if (hi == lo) return SA_OK;
    if (!ctx || !d_text || !d_keys_out || !code) return set_err(SA_E_INVALID, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SA_HIP(hipSetDevice(ctx->device));
    // the caller's code[] may be a temporary: stage it in the context's pinned
    // words and wait for the copy before returning
    uint16_t* h_code = reinterpret_cast<uint16_t*>(ctx->host_words + hw(kHwCode).at);
    std::memcpy(h_code, code, 512);
    SA_HIP(hipMemcpyAsync(ctx->code, h_code, 512, hipMemcpyHostToDevice, s));
    SA_HIP(host_sync(s));
    uint64_t top = 1;
    for (uint32_t t = 1; t < K; ++t) top *= base;
    const Chunking ch = plan_chunks(hi - lo);
    hipLaunchKernelGGL(k_pack_text, dim3(ch.chunks), dim3(kBlock), 0, s, d_text + lo, n - lo,
                       (const uint16_t*)ctx->code, ch, base, top, K, d_keys_out, (uint32_t*)nullptr, 0u,
                       (uint32_t*)nullptr);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

int sa_sort_pairs_device(sa_context* ctx, const uint64_t* d_keys_in, const uint32_t* d_vals_in, uint64_t m,
                         uint32_t bits, uint64_t* d_keys_out, uint32_t* d_vals_out, void* stream) {
    if (!ctx || !d_keys_in || !d_vals_in || !d_keys_out || !d_vals_out) return set_err(SA_E_INVALID, "NULL argument");
    if (bits == 0 || bits > 64) return set_err(SA_E_INVALID, "bits must be 1..64");
    if (m == 0) return SA_OK;
    if (m > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "m too large");
    if ((const void*)d_keys_in == (const void*)d_keys_out || (const void*)d_vals_in == (const void*)d_vals_out)
        return set_err(SA_E_INVALID, "outputs may not alias inputs");
    hipStream_t s = (hipStream_t)stream;
    SA_HIP(hipSetDevice(ctx->device));
    SA_TRY(ensure_capacity(ctx, m));
    ctx->radix = 0;
    SA_HIP(hipMemsetAsync(ctx->words, 0, 64, s));
    Run r{ctx, s, false, nullptr};
    const Chunking ch = plan_chunks(m);
    SrcKeys src{d_keys_in, d_vals_in};
    Sorted so;
    SA_TRY(radix_sort(r, src, 12 * m, ch, bits, SortBufs{d_vals_out, ctx->vals_alt, d_keys_out, ctx->keys[1]}, &so));
    if (so.keys != d_keys_out) SA_HIP(hipMemcpyAsync(d_keys_out, so.keys, m * 8, hipMemcpyDeviceToDevice, s));
    SA_READ(hwd, read_words(ctx, 20, s));
    if (hwd[kLookbackWord]) return set_err(SA_E_INTERNAL, "radix look-back did not complete");
    return SA_OK;
}

int sa_generate_text_device(uint8_t* d_out, uint64_t n, uint64_t seed, const uint8_t* alphabet, uint32_t sigma,
                            void* stream) {
    if (n == 0) return SA_OK;
    if (!d_out || !alphabet || sigma == 0 || sigma > 256) return set_err(SA_E_INVALID, "bad generator arguments");
    Alphabet a;
    std::memset(a.sym, 0, sizeof a.sym);
    std::memcpy(a.sym, alphabet, sigma);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, 16384);
    hipLaunchKernelGGL(k_gen_text, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, d_out, n, seed, a, sigma);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// ---- range-partitioned multi-GPU build (sa_dist.h) ----------------------
int sa_dist_begin(sa_context* ctx, const uint8_t* d_text, uint64_t n, int world, int rank,
                  const uint32_t present[8], uint64_t* d_coarse, void* stream, sa_dist_info* info) {
    if (!ctx || !info) return set_err(SA_E_INVALID, "NULL argument");
    return dist_begin(ctx, d_text, n, DistRank{world, rank}, present, d_coarse, (hipStream_t)stream, info);
}

int sa_dist_cuts(sa_context* ctx, const uint64_t* h_coarse, sa_dist_info* info) {
    if (!ctx || !info) return set_err(SA_E_INVALID, "NULL argument");
    return dist_cuts(ctx, h_coarse, info);
}

int sa_dist_reserve(sa_context* ctx, uint64_t max_n, int world) {
    if (!ctx) return set_err(SA_E_INVALID, "NULL argument");
    return dist_reserve(ctx, max_n, world);
}

int sa_dist_release(sa_context* ctx) {
    if (!ctx) return set_err(SA_E_INVALID, "NULL argument");
    SA_HIP(hipSetDevice(ctx->device));
    SA_HIP(hipDeviceSynchronize());
    free_dist(ctx);
    return SA_OK;
}

int sa_dist_plan_cuts(int world, uint64_t n, int bucket_bits, const uint64_t* h_coarse, uint32_t* cuts_out,
                      uint64_t* m_max) {
    if (world < 1 || world > kDistMaxWorld || !h_coarse || !cuts_out || !m_max)
        return set_err(SA_E_INVALID, "bad argument");
    if (bucket_bits < (int)kCoarseBits || bucket_bits > 32) return set_err(SA_E_INVALID, "bucket_bits out of range");
    std::vector<uint64_t> pre(kCoarse + 1, 0);
    for (uint32_t i = 0; i < kCoarse; ++i) pre[i + 1] = pre[i] + h_coarse[i];
    if (pre[kCoarse] != n) return set_err(SA_E_INVALID, "coarse histogram does not sum to n");
    const CutPlan cp = plan_cuts(world, n, (uint32_t)bucket_bits - kCoarseBits, pre.data(), cuts_out);
    *m_max = cp.mmax;
    return cp.ok ? SA_DIST_OK : SA_DIST_UNBALANCED;
}

int sa_dist_round1(sa_context* ctx, uint32_t* d_sa_local, void* stream, sa_dist_info* info, sa_stats* stats) {
    if (!ctx || !info) return set_err(SA_E_INVALID, "NULL argument");
    if (!ctx->dist) return set_err(SA_E_INVALID, "sa_dist_round1 before sa_dist_begin");
    Run r{ctx, (hipStream_t)stream, stats != nullptr, stats};
    return dist_round1(r, ctx->dist->text, d_sa_local, info);
}

int sa_dist_req_count(sa_context* ctx, uint64_t h, uint64_t* counts_out, void* stream, sa_dist_info* info) {
    if (!ctx || !counts_out || !info) return set_err(SA_E_INVALID, "NULL argument");
    return dist_req_count(ctx, h, counts_out, (hipStream_t)stream, info);
}

int sa_dist_req_fill(sa_context* ctx, uint64_t h, uint32_t* d_req, void* stream) {
    if (!ctx) return set_err(SA_E_INVALID, "NULL argument");
    return dist_req_fill(ctx, h, d_req, (hipStream_t)stream);
}

int sa_dist_answer(sa_context* ctx, const uint32_t* d_req, uint64_t nreq, uint64_t* d_ans, void* stream) {
    if (!ctx) return set_err(SA_E_INVALID, "NULL argument");
    return dist_answer(ctx, d_req, nreq, d_ans, (hipStream_t)stream);
}

int sa_dist_refine(sa_context* ctx, uint64_t h, const uint64_t* d_ans, uint32_t* d_sa_local, void* stream,
                   sa_dist_info* info) {
    if (!ctx || !info) return set_err(SA_E_INVALID, "NULL argument");
    return dist_refine(ctx, h, d_ans, d_sa_local, (hipStream_t)stream, info);
}

int sa_check(const uint8_t* text, uint64_t n, const void* sa, int sa_width) {
    return check_host(text, n, sa, sa_width);
}

}  // extern "C"
