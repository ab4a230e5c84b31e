// Host check of the arithmetic of the LCE index (hpc_suffix_array_amd/csrc/
// sa_lce.h) against brute force: the layout (sections in order, the size
// formula up to n = 2^32 - 1), and the query decomposition -- which masked
// block words and which cells of the two tables a rank range reads.  The index
// is built here by the tables' definitions, each section and the LCP array an
// exact-size heap buffer, so a build with -fsanitize=address sees any read past
// either end of a section; every touched word and cell is also asserted to lie
// inside.  Every interval for every n in 1 .. 200, structured intervals (ends
// at multiples of 64 and 4096 +- 1, the lengths 1, 2, 63 .. 65, 4095 .. 4097,
// 8192, (0, n)) at n around 4096, 8192 and 2^18; then lce and the substring
// order over all position pairs of small texts against direct comparison.
// Prints "ok <cases>" or the first mismatch.  Built by tests/test_lce_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "sa_lce.h"

typedef unsigned long long ull;
static long g_cases = 0;

#define FAIL(...)                         \
    do {                                  \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");                \
        return false;                     \
    } while (0)

struct Index {
    sa::LceHeader lay;
    uint64_t n;
    std::unique_ptr<uint32_t[]> lcp, blk, top;   // exactly n, 6 nb and levels ns words
};

static Index build(const std::vector<uint32_t>& lcp) {
    Index x;
    x.n = lcp.size();
    x.lay = sa::lce_layout(x.n);
    const uint64_t nb = x.lay.nb, ns = x.lay.ns;
    x.lcp.reset(new uint32_t[x.n]);
    std::copy(lcp.begin(), lcp.end(), x.lcp.get());
    x.blk.reset(new uint32_t[sa::kLceBlkLevels * nb]);
    x.top.reset(new uint32_t[(uint64_t)x.lay.levels * ns]);
    std::vector<uint32_t> bmin(nb, sa::kLceNone), smin(ns, sa::kLceNone);
    for (uint64_t r = 0; r < x.n; ++r) bmin[r / 64] = std::min(bmin[r / 64], lcp[r]);
    for (uint64_t b = 0; b < nb; ++b) smin[b / 64] = std::min(smin[b / 64], bmin[b]);
    for (uint32_t k = 0; k < sa::kLceBlkLevels; ++k)
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t end = std::min<uint64_t>({b + (1ull << k), (b / 64 + 1) * 64, nb});
            uint32_t m = sa::kLceNone;
            for (uint64_t c = b; c < end; ++c) m = std::min(m, bmin[c]);
            x.blk[k * nb + b] = m;
        }
    for (uint32_t k = 0; k < x.lay.levels; ++k)
        for (uint64_t s = 0; s < ns; ++s) {
            const uint64_t end = std::min<uint64_t>(s + (1ull << k), ns);
            uint32_t m = sa::kLceNone;
            for (uint64_t c = s; c < end; ++c) m = std::min(m, smin[c]);
            x.top[k * ns + s] = m;
        }
    return x;
}

// min lcp[x .. y] by the decomposition; false: something read lies outside its section
static bool answer(const Index& ix, uint64_t x, uint64_t y, uint32_t& out) {
    uint32_t m = sa::kLceNone;
    for (uint32_t which = 0; which < 2; ++which) {
        uint64_t block;
        uint32_t first, last;
        if (!sa::lce_partial(x, y, which, block, first, last)) continue;
        if (first > last || last >= 64) FAIL("partial %u of [%llu, %llu]: words %u .. %u", which, (ull)x, (ull)y, first, last);
        for (uint32_t w = first; w <= last; ++w) {
            const uint64_t r = block * 64 + w;
            if (r >= ix.n || r < x || r > y) FAIL("partial %u of [%llu, %llu] reads rank %llu", which, (ull)x, (ull)y, (ull)r);
            m = std::min(m, ix.lcp[r]);
        }
    }
    for (uint32_t slot = 0; slot < 8; ++slot) {
        bool top;
        uint64_t word;
        if (!sa::lce_cell(ix.lay, x, y, slot, top, word)) continue;
        if (slot >= 6) FAIL("slot %u used", slot);
        const uint64_t cap = top ? (uint64_t)ix.lay.levels * ix.lay.ns : (uint64_t)sa::kLceBlkLevels * ix.lay.nb;
        if (word >= cap) FAIL("cell %u of [%llu, %llu]: word %llu of %llu", slot, (ull)x, (ull)y, (ull)word, (ull)cap);
        m = std::min(m, top ? ix.top[word] : ix.blk[word]);
    }
    out = m;
    return true;
}

static std::vector<uint32_t> make_lcp(uint64_t n, int shape, std::mt19937_64& rng) {
    std::vector<uint32_t> v(n);
    for (uint64_t r = 0; r < n; ++r) {
        switch (shape) {
        case 0: v[r] = (uint32_t)(rng() % 4); break;               // ties everywhere
        case 1: v[r] = (uint32_t)r + 5; break;                     // the minimum is the first
        case 2: v[r] = (uint32_t)(n - r) + 5; break;               // the last
        default: v[r] = (uint32_t)rng() | 1u; break;               // all different, almost surely
        }
    }
    return v;
}

static bool check_all(uint64_t n, int shape, std::mt19937_64& rng) {
    const std::vector<uint32_t> lcp = make_lcp(n, shape, rng);
    const Index ix = build(lcp);
    for (uint64_t lo = 0; lo <= n; ++lo)
        for (uint64_t hi = 0; hi <= n + 1; ++hi) {
            uint64_t x, y;
            const bool has = sa::lce_interval_range(lo, hi, n, x, y);
            if (has != (lo < hi && hi <= n && hi - lo >= 2)) FAIL("range of [%llu, %llu) of %llu", (ull)lo, (ull)hi, (ull)n);
            if (!has) continue;
            uint32_t want = sa::kLceNone, got = 0;
            for (uint64_t r = lo + 1; r < hi; ++r) want = std::min(want, lcp[r]);
            if (!answer(ix, x, y, got)) return false;
            if (got != want) FAIL("n %llu shape %d [%llu, %llu): %u, want %u", (ull)n, shape, (ull)lo, (ull)hi, got, want);
            ++g_cases;
        }
    return true;
}

static bool check_structured(uint64_t n, int shape, std::mt19937_64& rng) {
    const std::vector<uint32_t> lcp = make_lcp(n, shape, rng);
    const Index ix = build(lcp);
    std::vector<uint64_t> pts = {0, 1, 2, n - 1, n - 2};
    auto around = [&](uint64_t c) {
        for (int d = -1; d <= 1; ++d)
            if ((int64_t)c + d >= 0 && c + d < n) pts.push_back(c + d);
    };
    for (uint64_t c = 0; c <= n; c += 4096) around(c);
    const uint64_t nb = ix.lay.nb;
    for (uint64_t k : {1ull, 2ull, 31ull, 32ull, 33ull, 63ull, 65ull, 127ull, (ull)nb / 2, (ull)nb - 2, (ull)nb - 1}) around(k * 64);
    for (int k = 0; k < 16; ++k) pts.push_back(rng() % n);
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    std::vector<uint8_t> mark(n, 0);
    for (uint64_t p : pts) mark[p] = 1;
    for (int k = 0; k < 64; ++k) mark[rng() % n] = 1;
    const uint64_t lens[] = {1, 2, 63, 64, 65, 4095, 4096, 4097, 8192};
    for (uint64_t x : pts) {
        uint32_t run = sa::kLceNone;
        for (uint64_t y = x; y < n; ++y) {
            run = std::min(run, lcp[y]);
            const uint64_t len = y - x + 1;
            if (!mark[y] && std::find(std::begin(lens), std::end(lens), len) == std::end(lens)) continue;
            uint32_t got = 0;
            if (!answer(ix, x, y, got)) return false;
            if (got != run) FAIL("n %llu shape %d [%llu, %llu]: %u, want %u", (ull)n, shape, (ull)x, (ull)y, got, run);
            ++g_cases;
        }
    }
    return true;
}

static bool check_layout() {
    const uint64_t ns[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 262144, 262145, 1ull << 20, (1ull << 28) + 3, 0xFFFFFFFFull};
    for (uint64_t n : ns) {
        const sa::LceHeader h = sa::lce_layout(n);
        const uint64_t nb = (n + 63) / 64, nsup = (nb + 63) / 64;
        uint32_t levels = 0;
        while ((1ull << levels) <= nsup && nsup) ++levels;   // floor(log2 ns) + 1
        const uint64_t want = (4096 + 4 * (6 * nb + levels * nsup) + 15) / 16 * 16;
        if (h.nb != nb || h.ns != nsup || h.levels != levels || h.bytes != want || sa::lce_index_bytes(n) != want)
            FAIL("layout of %llu: %llu bytes, want %llu", (ull)n, (ull)h.bytes, (ull)want);
        if (h.off_blk != 4096 || h.off_top != h.off_blk + 24 * nb || h.off_top + 4ull * levels * nsup > h.bytes)
            FAIL("sections of %llu", (ull)n);
        if (n >= (1ull << 20) && (double)h.bytes >= 0.40 * (double)n + 8192) FAIL("size of %llu", (ull)n);
        if (!sa::lce_header_ok(h, sa::lce_layout(n)) || sa::lce_header_ok(h, sa::lce_layout(n + 64))) FAIL("header check");
        ++g_cases;
    }
    return true;
}

// lce and the substring order by ISA, LCP and the decomposition against direct comparison
static bool check_text(const std::string& t) {
    const uint64_t n = t.size();
    std::vector<uint32_t> sfx(n), isa(n), lcp(n, 0);
    for (uint64_t i = 0; i < n; ++i) sfx[i] = (uint32_t)i;
    std::sort(sfx.begin(), sfx.end(), [&](uint32_t a, uint32_t b) { return t.compare(a, n, t, b, n) < 0; });
    for (uint64_t r = 0; r < n; ++r) isa[sfx[r]] = (uint32_t)r;
    auto direct = [&](uint64_t i, uint64_t j) {
        uint32_t l = 0;
        while (i + l < n && j + l < n && t[i + l] == t[j + l]) ++l;
        return l;
    };
    for (uint64_t r = 1; r < n; ++r) lcp[r] = direct(sfx[r - 1], sfx[r]);
    const Index ix = build(lcp);
    for (uint64_t i = 0; i <= n + 1; ++i)
        for (uint64_t j = 0; j <= n + 1; ++j) {
            uint32_t lce = 0;
            if (i < n && j < n) {
                if (i == j) {
                    lce = (uint32_t)(n - i);
                } else {
                    const uint64_t a = std::min(isa[i], isa[j]), b = std::max(isa[i], isa[j]);
                    if (!answer(ix, a + 1, b, lce)) return false;
                }
            }
            if (lce != direct(i, j)) FAIL("text %s: lce(%llu, %llu) = %u", t.c_str(), (ull)i, (ull)j, lce);
            ++g_cases;
            for (uint64_t li = 0; li <= n + 1; ++li)
                for (uint64_t lj = 0; lj <= n + 1; ++lj) {
                    const uint32_t ci = sa::lce_clip(i, li, n), cj = sa::lce_clip(j, lj, n);
                    int ord = sa::lce_order(lce, ci, cj);
                    if (ord == 2) ord = isa[i] < isa[j] ? -1 : 1;
                    const std::string a = i < n ? t.substr(i, li) : std::string(), b = j < n ? t.substr(j, lj) : std::string();
                    const int c = a.compare(b), want = c < 0 ? -1 : c > 0 ? 1 : 0;
                    if (ord != want)
                        FAIL("text %s: order of (%llu, %llu) and (%llu, %llu) = %d, want %d", t.c_str(), (ull)i, (ull)li, (ull)j,
                             (ull)lj, ord, want);
                    ++g_cases;
                }
        }
    return true;
}

int main() {
    std::mt19937_64 rng(12345);
    if (!check_layout()) return 1;
    for (uint64_t n = 1; n <= 200; ++n)
        for (int shape = 0; shape < 3; ++shape)
            if (!check_all(n, shape, rng)) return 1;
    for (uint64_t n : {4095ull, 4096ull, 4097ull, 8193ull, 262143ull, 262144ull, 262145ull})
        for (int shape : {0, 3})
            if (!check_structured(n, shape, rng)) return 1;
    for (const char* t : {"", "a", "aaaaaaa", "abababc", "banana", "abaababa", "abcabcab"})
        if (!check_text(t)) return 1;
    for (int k = 0; k < 6; ++k) {
        std::string t;
        const uint64_t n = 5 + rng() % 5;
        for (uint64_t i = 0; i < n; ++i) t.push_back("ab"[rng() & 1]);
        if (!check_text(t)) return 1;
    }
    std::printf("ok %ld\n", g_cases);
    return 0;
}
