// Host check of the host-compilable core of the k-mismatch search
// (hpc_suffix_array_amd/csrc/sa_hamming.h) against the definition: the piece
// bounds (directly and as the verify loop advances them), the count of the
// mismatching bytes of a word under every byte mask, the validity test with
// the clamp of a hit >= n, the verdict of every candidate (piece j, hit h) of
// texts of 0 .. 70 bytes over 1, 2, 4 and 256 symbols, and the argument itself:
// the candidates that the exact occurrences of the k + 1 pieces give, filtered
// by the rule, are the occurrences of the sliding-window definition, each
// exactly once, for k = 0 .. 5, m <= k and m = 0 included.  Texts and patterns
// are exact-size heap buffers, so a build with -fsanitize=address sees any read
// past either end; the word accessors abort on a read that starts at or past
// the end besides.  Prints "ok <cases>" or the first mismatch.  Built by
// tests/test_hamming_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <utility>
#include <vector>

#include "sa_hamming.h"

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

// ---- piece bounds ------------------------------------------------------------
static bool check_bounds(uint64_t m, uint32_t k) {
    std::vector<uint64_t> b(k + 2);
    for (uint32_t j = 0; j <= k + 1; ++j) {
        b[j] = sa::ham_piece_bound(m, k, j);
        const unsigned __int128 want = (unsigned __int128)j * m / (k + 1u);
        if ((unsigned __int128)b[j] != want) FAIL("bound m %llu k %u j %u", (ull)m, k, j);
    }
    if (b[0] != 0 || b[k + 1] != m) FAIL("bounds of m %llu k %u do not span the pattern", (ull)m, k);
    uint64_t empty = 0;
    for (uint32_t j = 0; j <= k; ++j) {
        if (b[j + 1] < b[j]) FAIL("bounds of m %llu k %u decrease at %u", (ull)m, k, j);
        empty += b[j + 1] == b[j];
    }
    const uint64_t want_empty = m < (uint64_t)k + 1 ? (uint64_t)k + 1 - m : 0;
    if (empty != want_empty) FAIL("m %llu k %u: %llu empty pieces, not %llu", (ull)m, k, (ull)empty, (ull)want_empty);
    if (want_empty && b[1] != 0) FAIL("m %llu k %u: piece 0 is not empty", (ull)m, k);
    // the verify loop's own bounds (no division per piece) are the same
    std::vector<std::pair<uint64_t, uint64_t>> seen;
    uint32_t dist = 99;
    const sa::HamVerdict v = sa::ham_verify_pieces(
        m, k, 0,
        [&](uint64_t lo, uint64_t hi, uint32_t) {
            seen.emplace_back(lo, hi);
            return 0u;
        },
        dist);
    if (v != sa::kHamKeep || dist != 0 || seen.size() != k + 1u) FAIL("verify loop m %llu k %u", (ull)m, k);
    for (uint32_t j = 0; j <= k; ++j)
        if (seen[j].first != b[j] || seen[j].second != b[j + 1]) FAIL("loop bounds m %llu k %u piece %u", (ull)m, k, j);
    ++g_cases;
    return true;
}

// ---- the word count -----------------------------------------------------------
static uint32_t naive_word(uint64_t a, uint64_t b, uint32_t sel) {
    uint32_t c = 0;
    for (int i = 0; i < 8; ++i)
        if (((sel >> i) & 1u) && ((a >> (8 * i)) & 0xFF) != ((b >> (8 * i)) & 0xFF)) ++c;
    return c;
}
static uint64_t byte_mask(uint32_t sel) {
    uint64_t m = 0;
    for (int i = 0; i < 8; ++i)
        if ((sel >> i) & 1u) m |= 0xFFull << (8 * i);
    return m;
}

static bool check_words(std::mt19937_64& rng) {
    for (int lane = 0; lane < 8; ++lane) {
        const uint64_t rest = rng() & ~(0xFFull << (8 * lane));
        for (uint32_t a = 0; a < 256; ++a)
            for (uint32_t b = 0; b < 256; ++b) {
                const uint64_t x = rest | ((uint64_t)a << (8 * lane)), y = rest | ((uint64_t)b << (8 * lane));
                const uint32_t want = a != b;
                if (sa::ham_word_mismatches(x ^ y, ~0ull) != want || sa::ham_word_mismatches(x ^ y, 0xFFull << (8 * lane)) != want ||
                    sa::ham_word_mismatches(x ^ y, ~(0xFFull << (8 * lane))) != 0 || sa::ham_word_mismatches(x ^ y, 0) != 0)
                    FAIL("word count lane %d bytes %u %u", lane, a, b);
                ++g_cases;
            }
    }
    const uint64_t special[] = {0ull, ~0ull, 0x8080808080808080ull, 0x7F7F7F7F7F7F7F7Full, 0x0101010101010101ull,
                                0xFF00FF00FF00FF00ull, 0x00000000000000FFull, 0xFF00000000000000ull};
    for (int rep = 0; rep < 600; ++rep) {
        const uint64_t a = rep < 8 ? special[rep] : rng(), b = rep % 3 == 0 ? (a ^ special[rep % 8]) : rng();
        for (uint32_t sel = 0; sel < 256; ++sel) {   // every mask, all-zero and all-ones among them
            if (sa::ham_word_mismatches(a ^ b, byte_mask(sel)) != naive_word(a, b, sel))
                FAIL("word count %llx %llx mask %x", (ull)a, (ull)b, sel);
            ++g_cases;
        }
    }
    for (uint64_t bytes = 0; bytes <= 20; ++bytes)
        if (sa::ham_low_mask(bytes) != byte_mask(bytes >= 8 ? 0xFFu : (1u << bytes) - 1u)) FAIL("low mask %llu", (ull)bytes);
    if (sa::ham_low_mask(~0ull) != ~0ull) FAIL("low mask of a long rest");
    return true;
}

// ---- the verify rule ------------------------------------------------------------
static uint32_t brute_dist(const Str& T, const Str& P, uint64_t p, uint64_t b, uint64_t e) {
    uint32_t d = 0;
    for (uint64_t t = b; t < e; ++t) d += T[p + t] != P[t];
    return d;
}

// every (k, j, h) of one text and pattern; hits past the text included
static bool check_pair(const Str& T, const Str& P, uint32_t kmax) {
    const uint64_t n = T.size, m = P.size;
    const Words tw = T.words(), pw = P.words();
    for (uint32_t k = 0; k <= kmax; ++k) {
        std::vector<uint64_t> b(k + 2);
        for (uint32_t j = 0; j <= k + 1; ++j) b[j] = (uint64_t)j * m / (k + 1u);
        // the sliding-window definition; the empty pattern occurs at [0, n)
        std::vector<std::pair<uint64_t, uint32_t>> want, got;
        for (uint64_t p = 0; p + m <= n && p < std::max<uint64_t>(n, 1) && n > 0; ++p) {
            const uint32_t d = brute_dist(T, P, p, 0, m);
            if (d <= k) want.emplace_back(p, d);
        }
        for (uint32_t j = 0; j <= k; ++j)
            for (uint64_t h = 0; h < n + 3; ++h) {
                uint64_t p = ~0ull;
                uint32_t dist = 999;
                const sa::HamVerdict v = sa::ham_verify(n, m, k, j, h, tw, pw, p, dist);
                ++g_cases;
                const bool valid = h < n && h >= b[j] && h - b[j] + m <= n;
                if (!valid) {   // on both sides: h < b_j, p + m > n; and the clamp of h >= n
                    if (v != sa::kHamInvalid) FAIL("n %llu m %llu k %u j %u h %llu is invalid", (ull)n, (ull)m, k, j, (ull)h);
                    continue;
                }
                const uint64_t p0 = h - b[j];
                if (v == sa::kHamInvalid || p != p0) FAIL("n %llu m %llu k %u j %u h %llu is valid", (ull)n, (ull)m, k, j, (ull)h);
                const uint32_t d = brute_dist(T, P, p0, 0, m);
                uint32_t first = k + 1;
                for (uint32_t jj = 0; jj <= k && first > k; ++jj)
                    if (brute_dist(T, P, p0, b[jj], b[jj + 1]) == 0) first = jj;
                const bool keep = d <= k && first == j;
                if (keep != (v == sa::kHamKeep))
                    FAIL("n %llu m %llu k %u j %u h %llu: verdict %d, d %u first %u", (ull)n, (ull)m, k, j, (ull)h, (int)v, d, first);
                if (keep && dist != d) FAIL("n %llu m %llu k %u j %u h %llu: distance %u, not %u", (ull)n, (ull)m, k, j, (ull)h, dist, d);
                if (!keep && dist != 999) FAIL("a distance was written for a candidate that is not kept");
                if (v == sa::kHamDuplicate && !(first < j)) FAIL("duplicate without an earlier exact piece");
                if (v == sa::kHamNoSeed && brute_dist(T, P, p0, b[j], b[j + 1]) == 0) FAIL("no seed, but piece %u matches", j);
                // a candidate of the pipeline: h is an exact occurrence of piece j (an empty piece: every h < n)
                if (brute_dist(T, P, p0, b[j], b[j + 1]) == 0 && keep) got.emplace_back(p0, dist);
            }
        std::sort(got.begin(), got.end());
        if (got != want)
            FAIL("n %llu m %llu k %u: %llu kept, %llu occurrences", (ull)n, (ull)m, k, (ull)got.size(), (ull)want.size());
        ++g_cases;
    }
    return true;
}

static std::vector<uint8_t> rand_str(std::mt19937_64& rng, uint64_t len, const std::vector<uint8_t>& sym) {
    std::vector<uint8_t> v(len);
    for (auto& c : v) c = sym.empty() ? (uint8_t)rng() : sym[rng() % sym.size()];
    return v;
}

int main() {
    std::mt19937_64 rng(20240521);
    // piece bounds: every (m, k) with m <= 70 and k <= 9, plus k = 255; the arithmetic at m = 2^32 - 1
    for (uint64_t m = 0; m <= 70; ++m) {
        for (uint32_t k = 0; k <= 9; ++k)
            if (!check_bounds(m, k)) return 1;
        if (!check_bounds(m, 255)) return 1;
    }
    for (uint64_t m : {0xFFFFFFFFull, 0xFFFFFFFEull, 0xFFFFFF00ull, 0x100000000ull, 256ull, 255ull, 257ull, 1000003ull})
        for (uint32_t k : {0u, 1u, 2u, 254u, 255u})
            if (!check_bounds(m, k)) return 1;
    if (sa::ham_piece_bound(0xFFFFFFFFull, 255, 255) != 0xFFFFFFFFull * 255 / 256) {
        std::printf("FAIL the product needs 64 bits\n");
        return 1;
    }
    if (!check_words(rng)) return 1;
    // the clamp: a hit at or past n is no candidate, whatever else holds
    for (uint64_t h : {10ull, 11ull, 0xFFFFFFFFull, ~0ull}) {
        uint64_t p = 0;
        if (sa::ham_candidate_start(h, 0, 0, 10, p) || sa::ham_candidate_start(h, 0, 1, 10, p) ||
            sa::ham_candidate_start(h, 3, 5, 10, p)) {
            std::printf("FAIL a hit at %llu of 10 counts\n", (ull)h);
            return 1;
        }
    }
    {
        uint64_t p = 99;
        if (!sa::ham_candidate_start(9, 0, 1, 10, p) || p != 9 || sa::ham_candidate_start(9, 0, 2, 10, p) ||
            !sa::ham_candidate_start(9, 9, 10, 10, p) || p != 0 || sa::ham_candidate_start(9, 9, 11, 10, p) ||
            sa::ham_candidate_start(2, 3, 4, 10, p) || sa::ham_candidate_start(0, 0, ~0ull, 10, p)) {
            std::printf("FAIL candidate start\n");
            return 1;
        }
    }
    // the verify rule over 1, 2, 4 and 256 symbols, 0x00 and 0xFF among them
    const std::vector<std::vector<uint8_t>> alphabets = {{'a'}, {0x00, 0xFF}, {'A', 'C', 'G', 'T'}, {}};
    for (const auto& sym : alphabets)
        for (int rep = 0; rep < 130; ++rep) {
            const uint64_t n = rep < 71 ? (uint64_t)rep : rng() % 71;
            const std::vector<uint8_t> t = rand_str(rng, n, sym);
            uint64_t m = rep % 5 == 4 ? rng() % 71 : rng() % 14;
            std::vector<uint8_t> p;
            if (rep % 3 != 0 && n >= m && n > 0) {   // cut from the text, with a few substitutions
                const uint64_t at = rng() % (n - m + 1);
                p.assign(t.begin() + at, t.begin() + at + m);
                for (uint64_t s = rng() % 4; s > 0 && m > 0; --s) {
                    const uint64_t x = rng() % m;
                    p[x] = sym.empty() ? (uint8_t)(p[x] ^ (1u << (rng() % 8))) : sym[rng() % sym.size()];
                }
            } else {
                if (rep % 9 == 0) m = n + 1 + rng() % 3;   // m > n
                p = rand_str(rng, m, sym);
            }
            if (!check_pair(Str(t), Str(p), 5)) return 1;
        }
    // the corners by hand: the empty pattern, the empty text, m <= k, ends of the text
    for (const char* ts : {"", "a", "ab", "banana", "aaaaaaaaaaaaaaaaaaaaaaaa", "abababababababababab"})
        for (const char* ps : {"", "a", "b", "an", "aa", "ana", "nab", "aaaaaaaaa", "ababababab", "bananas"}) {
            const std::vector<uint8_t> t(ts, ts + std::strlen(ts)), p(ps, ps + std::strlen(ps));
            if (!check_pair(Str(t), Str(p), 5)) return 1;
        }
    std::printf("ok %ld\n", g_cases);
    return 0;
}
