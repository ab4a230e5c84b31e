// Host check of the host-compilable core of the maximal exact matches
// (hpc_suffix_array_amd/csrc/sa_mem.h) against brute force: the right
// extension by 8-byte words (whole, from a seed of L bytes, and with a budget
// of words), the left check, the seed rule, the clamp of an SA entry >= n, and
// the compaction argument itself (seed hits that are left-maximal, extended,
// are exactly the MEMs of the definition).  Texts and queries are exact-size
// heap buffers of 0 .. 70 bytes, random and of one symbol, and every (i, p) is
// tried, so the ends fall on every offset of a word and a build with
// -fsanitize=address sees any read past either end; the word accessors abort
// on a read at or past the end besides.  The arithmetic at n = m = 2^32 - 1
// runs on accessors with no memory behind them.  Prints "ok <cases>" or the
// first mismatch.  Built by tests/test_mem_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <tuple>
#include <vector>

#include "sa_mem.h"

typedef unsigned long long ull;
static long g_cases = 0;

#define FAIL(...)                         \
    do {                                  \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");                \
        return false;                     \
    } while (0)

// little-endian 8 bytes at x, zero past the end; a read that starts at or past the end is a bug of the caller
struct Words {
    const uint8_t* p;
    uint64_t size;
    uint64_t operator()(uint64_t x) const {
        if (x >= size) {
            std::printf("FAIL word read at %llu of %llu\n", (ull)x, (ull)size);
            std::abort();
        }
        uint64_t w = 0;
        for (uint64_t b = 0; b < 8 && x + b < size; ++b) w |= (uint64_t)p[x + b] << (8 * b);
        return w;
    }
};

struct Str {
    std::unique_ptr<uint8_t[]> heap;   // exactly size bytes
    uint64_t size;
    Str(const std::vector<uint8_t>& v) : heap(new uint8_t[v.size()]), size(v.size()) {
        if (size) std::memcpy(heap.get(), v.data(), size);
    }
    uint8_t operator[](uint64_t i) const { return heap[i]; }
    Words words() const { return Words{heap.get(), size}; }
};

static uint64_t brute(const Str& Q, uint64_t i, const Str& T, uint64_t p) {
    uint64_t k = 0;
    while (i + k < Q.size && p + k < T.size && Q[i + k] == T[p + k]) ++k;
    return k;
}

static bool check_pair(const Str& T, const Str& Q) {
    const uint64_t n = T.size, m = Q.size;
    const Words tw = T.words(), qw = Q.words();
    for (uint64_t i = 0; i <= m; ++i)
        for (uint64_t p = 0; p <= n; ++p) {   // i == m and p == n: the empty suffixes
            const uint64_t want = brute(Q, i, T, p);
            const uint64_t got = sa::mem_extend(i, p, 0, n, m, tw, qw);
            if (got != want) FAIL("extend n %llu m %llu i %llu p %llu: %llu, not %llu", (ull)n, (ull)m, (ull)i, (ull)p,
                                  (ull)got, (ull)want);
            ++g_cases;
            for (uint64_t L = 1; L <= 9 && L <= want; ++L) {
                if (sa::mem_extend(i, p, L, n, m, tw, qw) != want)
                    FAIL("extend from %llu n %llu m %llu i %llu p %llu", (ull)L, (ull)n, (ull)m, (ull)i, (ull)p);
                for (uint64_t budget = 0; budget <= 2; ++budget) {
                    bool done = false;
                    const uint64_t k = sa::mem_extend_steps(i, p, L, n, m, tw, qw, budget, done);
                    if (done ? k != want : (k != L + 8 * budget || k > want))
                        FAIL("budget %llu from %llu n %llu m %llu i %llu p %llu: %llu done %d, whole %llu", (ull)budget,
                             (ull)L, (ull)n, (ull)m, (ull)i, (ull)p, (ull)k, (int)done, (ull)want);
                }
                ++g_cases;
            }
            if (i < m && p < n) {
                const uint8_t qb = i ? Q[i - 1] : 0, tb = p ? T[p - 1] : 0;
                const bool left = !(i > 0 && p > 0 && Q[i - 1] == T[p - 1]);
                // at i == 0 or p == 0 the bytes passed do not count
                if (sa::mem_left_maximal(i, p, qb, tb) != left || (i == 0 && !sa::mem_left_maximal(i, p, 7, 7)) ||
                    (p == 0 && !sa::mem_left_maximal(i, p, 7, 7)))
                    FAIL("left check i %llu p %llu", (ull)i, (ull)p);
            }
        }
    return true;
}

// the MEMs by the definition against the MEMs by the core: the hits of every
// position's seed (all p with L shared bytes: what the SA interval of the seed
// lists), filtered by max_occ through the seed rule, kept when left-maximal,
// extended from L
typedef std::tuple<uint64_t, uint64_t, uint64_t> Mem;
static bool check_mems(const Str& T, const Str& Q, uint64_t L, uint64_t max_occ) {
    const uint64_t n = T.size, m = Q.size;
    const Words tw = T.words(), qw = Q.words();
    std::vector<Mem> want, got;
    uint64_t want_skipped = 0, got_skipped = 0;
    for (uint64_t i = 0; i < m; ++i) {
        uint64_t occ = 0;
        for (uint64_t p = 0; p < n; ++p) occ += brute(Q, i, T, p) >= L ? 1 : 0;
        const bool drop = max_occ && occ > max_occ;
        want_skipped += drop ? 1 : 0;
        for (uint64_t p = 0; p < n && !drop; ++p) {
            const uint64_t l = brute(Q, i, T, p);
            if (l >= L && !(i > 0 && p > 0 && Q[i - 1] == T[p - 1])) want.emplace_back(i, p, l);
        }
        // the core: len = the longest match under the cap L, [lo, hi) of occ entries somewhere in the SA
        uint64_t len = 0;
        for (uint64_t p = 0; p < n; ++p) len = std::max(len, std::min(brute(Q, i, T, p), L));
        bool skipped;
        const uint64_t lo = 3, c = sa::mem_seed_count(len, lo, lo + (len == L ? occ : n), n + 3, L, max_occ, skipped);
        got_skipped += skipped ? 1 : 0;
        if (c == 0) continue;
        if (c != occ) FAIL("seed count %llu of %llu occurrences", (ull)c, (ull)occ);
        for (uint64_t p = 0; p < n; ++p)
            if (brute(Q, i, T, p) >= L && sa::mem_left_maximal(i, p, i ? Q[i - 1] : 0, p ? T[p - 1] : 0))
                got.emplace_back(i, p, sa::mem_extend(i, p, L, n, m, tw, qw));
    }
    if (want != got || want_skipped != got_skipped)
        FAIL("MEMs n %llu m %llu L %llu max_occ %llu: %zu, not %zu", (ull)n, (ull)m, (ull)L, (ull)max_occ, got.size(),
             want.size());
    for (const Mem& x : want) {   // maximal to the right, by the definition
        const uint64_t i = std::get<0>(x), p = std::get<1>(x), l = std::get<2>(x);
        if (!(i + l == m || p + l == n || Q[i + l] != T[p + l])) FAIL("a MEM extends to the right");
    }
    g_cases += (long)want.size() + 1;
    return true;
}

static bool check_seed_rule() {
    bool sk = true;
    // no seed: the longest match is shorter than L
    if (sa::mem_seed_count(3, 0, 10, 10, 4, 0, sk) != 0 || sk) FAIL("len < L");
    if (sa::mem_seed_count(4, 2, 9, 10, 4, 0, sk) != 7 || sk) FAIL("a seed with 7 hits");
    if (sa::mem_seed_count(4, 2, 9, 10, 4, 7, sk) != 7 || sk) FAIL("max_occ == hits keeps them");
    if (sa::mem_seed_count(4, 2, 9, 10, 4, 6, sk) != 0 || !sk) FAIL("max_occ below the hits skips");
    if (sa::mem_seed_count(3, 2, 9, 10, 4, 6, sk) != 0 || sk) FAIL("no seed is not a skip");
    // intervals that break lo <= hi <= n are empty and no skip
    if (sa::mem_seed_count(4, 5, 4, 10, 4, 1, sk) != 0 || sk) FAIL("lo > hi");
    if (sa::mem_seed_count(4, 0, 11, 10, 4, 1, sk) != 0 || sk) FAIL("hi > n");
    const uint64_t big = 0xFFFFFFFFull;
    if (sa::mem_seed_count(big, 0, big, big, big, 0, sk) != 0xFFFFFFFFu || sk) FAIL("whole SA at n = 2^32 - 1");
    if (sa::mem_seed_count(1, 0, big, big, 1, 1ull << 40, sk) != 0xFFFFFFFFu || sk) FAIL("max_occ above 2^32");
    g_cases += 9;
    return true;
}

static bool check_clamp() {
    if (sa::mem_clamp_pos(0, 1) != 0 || sa::mem_clamp_pos(1, 1) != 0 || sa::mem_clamp_pos(9, 10) != 9 ||
        sa::mem_clamp_pos(10, 10) != 9 || sa::mem_clamp_pos(0xFFFFFFFFull, 10) != 9 ||
        sa::mem_clamp_pos(0xFFFFFFFFull, 0xFFFFFFFFull) != 0xFFFFFFFEull)
        FAIL("clamp");
    // an SA entry >= n that reaches the extension unclamped is the empty suffix: no word is read
    const Str T(std::vector<uint8_t>(10, 'a')), Q(std::vector<uint8_t>(10, 'a'));
    for (uint64_t p : {(uint64_t)10, (uint64_t)11, (uint64_t)0xFFFFFFFFull, ~(uint64_t)0})
        for (uint64_t start : {0, 4})
            if (sa::mem_extend(0, p, start, 10, 10, T.words(), Q.words()) != 0) FAIL("extension at p >= n");
    // clamped: the last byte of the text, one byte to share at most
    if (sa::mem_extend(0, sa::mem_clamp_pos(99, 10), 0, 10, 10, T.words(), Q.words()) != 1) FAIL("extension at n - 1");
    // a start past the shared end (an SA that is none): the result is the end, nothing is read
    if (sa::mem_extend(8, 9, 5, 10, 10, T.words(), Q.words()) != 1) FAIL("start past lim");
    g_cases += 12;
    return true;
}

// n = m = 2^32 - 1 with no memory behind the accessors: the text is a formula
// of the position, the query is the text shifted by `shift` with one byte
// changed at query position `bad`.
static const uint64_t kBig = 0xFFFFFFFFull;
static uint8_t big_byte(uint64_t x) { return (uint8_t)((x * 2654435761ull) >> 13); }
struct BigText {
    uint64_t operator()(uint64_t x) const {
        if (x >= kBig) {
            std::printf("FAIL text word at %llu\n", (ull)x);
            std::abort();
        }
        uint64_t w = 0;
        for (uint64_t b = 0; b < 8 && x + b < kBig; ++b) w |= (uint64_t)big_byte(x + b) << (8 * b);
        return w;
    }
};
struct BigQuery {
    uint64_t shift, bad;
    uint64_t operator()(uint64_t y) const {
        if (y >= kBig) {
            std::printf("FAIL query word at %llu\n", (ull)y);
            std::abort();
        }
        uint64_t w = 0;
        for (uint64_t b = 0; b < 8 && y + b < kBig; ++b)
            w |= (uint64_t)(uint8_t)(big_byte(y + b + shift) ^ (y + b == bad ? 0x5A : 0)) << (8 * b);
        return w;
    }
};

static bool check_big() {
    const BigText tw;
    for (uint64_t shift : {0, 1, 5, 1000})
        for (uint64_t back : {1, 7, 8, 9, 64, 1000, 4099}) {
            // Q[i + k] == T[i + shift + k]: from p = i + shift the two agree to the text's end
            const uint64_t p = kBig - back, i = p - shift;
            const BigQuery clean{shift, ~0ull};
            if (sa::mem_extend(i, p, 0, kBig, kBig, tw, clean) != back)
                FAIL("2^32 - 1: the end of the text, shift %llu back %llu", (ull)shift, (ull)back);
            if (sa::mem_extend(i, p, back > 3 ? 3 : 0, kBig, kBig, tw, clean) != back) FAIL("2^32 - 1: from a seed");
            // the query's end comes first when the text is ahead of it
            if (sa::mem_extend(p, i, 0, kBig, kBig, BigQuery{0, ~0ull}, BigQuery{shift, ~0ull}) > back)
                FAIL("2^32 - 1: past the query's end");
            for (uint64_t at : {(uint64_t)0, (uint64_t)1, back / 2, back - 1}) {
                const BigQuery q{shift, i + at};
                if (sa::mem_extend(i, p, 0, kBig, kBig, tw, q) != at)
                    FAIL("2^32 - 1: mismatch at %llu of %llu", (ull)at, (ull)back);
                ++g_cases;
            }
            g_cases += 3;
        }
    return true;
}

int main() {
    std::mt19937_64 rng(12345);
    if (!check_seed_rule() || !check_clamp() || !check_big()) return 1;
    for (int kind = 0; kind < 3; ++kind)   // two symbols, four symbols with 0x00 and 0xFF, one symbol
        for (uint64_t n = 0; n <= 70; ++n) {
            std::vector<uint64_t> ms = {0, 1, 8, 70, n};
            for (int k = 0; k < 4; ++k) ms.push_back(rng() % 71);
            for (uint64_t m : ms) {
                static const uint8_t sym[4] = {0x00, 0xFF, 'a', 'b'};
                auto gen = [&](uint64_t len) {
                    std::vector<uint8_t> v(len);
                    for (auto& x : v) x = kind == 2 ? 'a' : kind == 0 ? (uint8_t)('a' + rng() % 2) : sym[rng() % 4];
                    return v;
                };
                std::vector<uint8_t> t = gen(n), q = gen(m);
                // a copied block, so that long matches with ends inside the strings occur
                if (kind != 2 && n > 20 && m > 20) {
                    const uint64_t len = 9 + rng() % 11, a = rng() % (n - len), b = rng() % (m - len);
                    std::copy(t.begin() + a, t.begin() + a + len, q.begin() + b);
                }
                const Str T(t), Q(q);
                if (!check_pair(T, Q)) return 1;
                if (n % 3 == 0)
                    for (uint64_t L = 1; L <= 9; ++L)
                        for (uint64_t occ : {0, 1, 5})
                            if (!check_mems(T, Q, L, occ)) return 1;
            }
        }
    std::printf("ok %ld\n", g_cases);
    return 0;
}
