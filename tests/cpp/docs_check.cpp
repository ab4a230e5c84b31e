// Host check of the arithmetic of the document collections (hpc_suffix_array_amd/
// csrc/sa_docs.h) against brute force: the boundary search doc_search on
// random collections with empty documents at every place (first, last, runs
// in the middle, all but one) and on accessors with no memory behind them
// (D = 2^32 - 2), the PRV <= lo predicate against a direct count of distinct
// documents on random document arrays, the capped count, the class and the
// chunks of a query, and the key width chosen for D.  The offset arrays are
// exact-size heap buffers of D entries (the search may not read doc_off[D]), so
// a build with -fsanitize=address sees any read past either end.  Prints
// "ok <cases>" or the first mismatch.  Built by tests/test_docs_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "sa_docs.h"

typedef unsigned long long ull;
static long g_cases = 0;

#define FAIL(...)                         \
    do {                                  \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");                \
        return false;                     \
    } while (0)

struct HeapOff {
    const uint64_t* p;
    uint64_t size;   // D: entry D (= n) is never read
    uint64_t operator()(uint64_t i) const {
        if (i >= size) {
            std::printf("FAIL offset %llu read of %llu\n", (ull)i, (ull)size);
            std::abort();
        }
        return p[i];
    }
};

// the largest d with off[d] <= p, by a scan from the back
static uint32_t brute_doc(const std::vector<uint64_t>& off, uint64_t p) {
    for (uint64_t d = off.size() - 1; d-- > 0;)
        if (off[d] <= p) return (uint32_t)d;
    return 0;
}

static bool check_collection(const std::vector<uint64_t>& off, const char* what) {
    const uint64_t D = off.size() - 1, n = off[D];
    std::unique_ptr<uint64_t[]> heap(new uint64_t[D]);   // exactly D entries
    std::copy(off.begin(), off.begin() + D, heap.get());
    const HeapOff acc{heap.get(), D};
    for (uint64_t p = 0; p < n; ++p) {
        const uint32_t got = sa::doc_search(acc, D, p), want = brute_doc(off, p);
        if (got != want) FAIL("%s: doc(%llu) = %u, want %u", what, (ull)p, got, want);
        if (off[got] > p || off[got + 1] <= p) FAIL("%s: doc(%llu) = %u does not hold it", what, (ull)p, got);
        ++g_cases;
    }
    // positions at and past n stay inside [0, D) (the kernels give SA_DOC_NONE before they search)
    for (uint64_t p : {n, n + 5, (uint64_t)0xFFFFFFFFull})
        if (sa::doc_search(acc, D, p) >= D) FAIL("%s: doc(%llu) is not below D", what, (ull)p);
    return true;
}

static bool check_search() {
    std::mt19937_64 rng(2024);
    for (int round = 0; round < 600; ++round) {
        const uint64_t D = 1 + rng() % (round % 3 == 0 ? 5 : 70);
        const uint64_t n = rng() % 200;
        std::vector<uint64_t> off(D + 1);
        off[0] = 0;
        off[D] = n;
        for (uint64_t d = 1; d < D; ++d) off[d] = n ? rng() % (n + 1) : 0;
        std::sort(off.begin(), off.end());
        const int kind = round % 6;
        // empty documents forced at the front, at the back, in a run of three
        if (kind == 1 && D > 2) off[1] = 0;
        if (kind == 2 && D > 2) off[D - 1] = n;
        if (kind == 3 && D > 5) off[D / 2 + 1] = off[D / 2 + 2] = off[D / 2];
        if (kind == 4 && D > 3) {   // one document holds all but two positions
            std::fill(off.begin() + 1, off.end() - 1, n >= 2 ? 1 : 0);
            off[D - 1] = n >= 2 ? n - 1 : n;
            std::sort(off.begin(), off.end());
        }
        if (kind == 5)   // every document but the last is empty
            std::fill(off.begin(), off.end() - 1, 0);
        std::sort(off.begin(), off.end());
        char what[32];
        std::snprintf(what, sizeof what, "random %d", round);
        if (!check_collection(off, what)) return false;
    }
    if (!check_collection({0, 1}, "one byte")) return false;
    if (!check_collection({0, 0, 0, 0, 7}, "empties first")) return false;
    if (!check_collection({0, 7, 7, 7, 7}, "empties last")) return false;
    if (!check_collection({0, 0}, "empty text")) return false;
    // garbage offsets (not sorted, above n): the result stays inside [0, D)
    for (int round = 0; round < 200; ++round) {
        const uint64_t D = 1 + rng() % 40;
        std::unique_ptr<uint64_t[]> heap(new uint64_t[D]);
        for (uint64_t d = 0; d < D; ++d) heap[d] = rng();
        const HeapOff acc{heap.get(), D};
        for (int k = 0; k < 20; ++k) {
            if (sa::doc_search(acc, D, rng()) >= D) FAIL("garbage offsets: a document past D");
            ++g_cases;
        }
    }
    return true;
}

// off(d) computed, nothing stored: documents of `len` bytes, D up to 2^32 - 2
struct SynthOff {
    uint64_t len;
    uint64_t operator()(uint64_t d) const { return d * len; }
};

static bool check_synthetic() {
    std::mt19937_64 rng(5);
    const uint64_t Ds[] = {1, 2, 255, 256, 257, 65536, 65537, sa::kDocMaxDocs};
    for (uint64_t D : Ds)
        for (uint64_t len : {(uint64_t)1, (uint64_t)3}) {
            if (D * len > 0xFFFFFFFFull) continue;
            const SynthOff off{len};
            const uint64_t n = D * len;
            for (int k = 0; k < 300; ++k) {
                const uint64_t p = k == 0 ? 0 : k == 1 ? n - 1 : rng() % n;
                if (sa::doc_search(off, D, p) != p / len) FAIL("synthetic D %llu len %llu p %llu", (ull)D, (ull)len, (ull)p);
                ++g_cases;
            }
        }
    return true;
}

// the PRV predicate counts the distinct documents of every interval
static bool check_prev() {
    std::mt19937_64 rng(77);
    for (int round = 0; round < 300; ++round) {
        const uint32_t n = 1 + (uint32_t)(rng() % 60), D = 1 + (uint32_t)(rng() % (round % 2 ? 4 : 40));
        std::vector<uint32_t> da(n), prv(n);
        std::vector<uint32_t> last(D, 0);
        for (uint32_t r = 0; r < n; ++r) {
            da[r] = (uint32_t)(rng() % D);
            prv[r] = last[da[r]];
            last[da[r]] = r + 1;
        }
        for (uint32_t lo = 0; lo <= n; ++lo)
            for (uint32_t hi = lo; hi <= n; ++hi) {
                std::set<uint32_t> want(da.begin() + lo, da.begin() + hi);
                std::vector<uint32_t> firsts;
                for (uint32_t r = lo; r < hi; ++r)
                    if (sa::doc_first(prv[r], lo)) firsts.push_back(da[r]);
                if (firsts.size() != want.size()) FAIL("df of [%u, %u): %zu, want %zu", lo, hi, firsts.size(), want.size());
                if (std::set<uint32_t>(firsts.begin(), firsts.end()) != want) FAIL("the first ranks of [%u, %u)", lo, hi);
                ++g_cases;
            }
    }
    // the widest values
    if (!sa::doc_first(0, 0) || sa::doc_first(1, 0) || !sa::doc_first(0xFFFFFFFFu, 0xFFFFFFFFull) ||
        sa::doc_first(0xFFFFFFFFu, 0xFFFFFFFEull))
        FAIL("doc_first at the ends");
    return true;
}

static bool check_counts() {
    const uint64_t T = sa::kDocTile, G = sa::kDocGroupMax;
    const uint64_t dfs[] = {0, 1, 2, T - 1, T, T + 1, 0xFFFFFFFFull};
    const uint64_t caps[] = {0, 1, 2, T, T + 1, 1ull << 40};
    for (uint64_t df : dfs)
        for (uint64_t cap : caps) {
            const uint64_t want = cap ? std::min(df, cap) : df;
            if (sa::doc_capped(df, cap) != want) FAIL("capped %llu cap %llu", (ull)df, (ull)cap);
            ++g_cases;
        }
    const uint64_t lens[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, G - 1, G, G + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1,
                             3 * T + 5, 0xFFFFFFFFull};
    for (uint64_t len : lens) {
        const uint32_t want = len == 0 ? 0u : len <= G ? 1u : 2u;
        if (sa::doc_class(len) != want) FAIL("class of %llu", (ull)len);
        // chunks: every rank of a tiled interval in exactly one chunk of at most T ranks
        const uint64_t ch = sa::doc_chunks(len);
        if (want != 2u ? ch != 0 : (ch * T < len || (ch - 1) * T >= len)) FAIL("chunks of %llu: %llu", (ull)len, (ull)ch);
        ++g_cases;
    }
    if (sa::kDocEmpty != 0 || sa::kDocGroupClass != 1 || sa::kDocTiledClass != 2) FAIL("class numbers");
    // an interval that breaks lo <= hi <= n is empty
    if (sa::doc_class(sa::locate_count(5, 4, 10, 0)) != sa::kDocEmpty || sa::doc_class(sa::locate_count(0, 11, 10, 0)) != sa::kDocEmpty)
        FAIL("an invalid interval has a class");
    return true;
}

static bool check_key_bits() {
    const uint64_t Ds[] = {1, 2, 3, 4, 5, 255, 256, 257, 65535, 65536, 65537, 1ull << 31, sa::kDocMaxDocs};
    const uint32_t want[] = {1, 1, 2, 2, 3, 8, 8, 9, 16, 16, 17, 31, 32};
    for (int k = 0; k < 13; ++k) {
        const uint32_t b = sa::doc_key_bits(Ds[k]);
        if (b != want[k]) FAIL("key bits of D = %llu: %u, want %u", (ull)Ds[k], b, want[k]);
        // every id below D fits, and one bit less would not (above one bit)
        if (b < 64 && ((Ds[k] - 1) >> b)) FAIL("id %llu does not fit %u bits", (ull)(Ds[k] - 1), b);
        if (b > 1 && !((Ds[k] - 1) >> (b - 1))) FAIL("%u bits are one too many for D = %llu", b, (ull)Ds[k]);
        ++g_cases;
    }
    return true;
}

int main() {
    if (!check_search() || !check_synthetic() || !check_prev() || !check_counts() || !check_key_bits()) return 1;
    std::printf("ok %ld\n", g_cases);
    return 0;
}
