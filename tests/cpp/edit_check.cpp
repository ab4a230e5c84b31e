// Host check of the host-compilable core of the k-difference search
// (hpc_suffix_array_amd/csrc/sa_edit.h) against the plain full DP (Sellers):
//   - the union of the masks over the seeds of a pattern (every exact occurrence
//     of each of its k + 1 pieces) is exactly { e : D(e) <= k };
//   - the mask of one band is exactly the DP restricted to the diagonals
//     c - k .. c + k and the columns [0, n] with a free start in row 0, for seed
//     diagonals and for diagonals that are clipped at 0 and at n;
//   - the backward finish gives D(e) and the largest start of every such end;
//   - a hit >= n and a pattern with m <= k give no end.
// Every text over {a, b} with n <= 9 against every pattern with m <= 5 and
// k <= 3, and random cases over 2 .. 4 symbols (and bytes 0x00 / 0xFF) up to
// n = 80, m = 70, k = 31, with m > n, m = k + 1 and k = 31 among them.  Texts
// and patterns are exact-size heap buffers, so a build with -fsanitize=address
// sees any read past either end; the word accessors abort on a read that starts
// at or past the end besides.  Prints "ok <checks>" or the first mismatch.
// Built by tests/test_edit_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "sa_edit.h"

typedef unsigned long long ull;
static long g_checks = 0;

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

static const int kInf = 1 << 20;

// D(e), e in [0, n], and best[e]: the largest start of an optimal alignment that ends at e (ties keep the
// larger start; row 0 starts where it stands)
static void sellers(const Str& T, const Str& P, std::vector<int>& D, std::vector<int64_t>& best) {
    const int64_t n = (int64_t)T.size, m = (int64_t)P.size;
    std::vector<int> row(n + 1, 0), cur(n + 1);
    std::vector<int64_t> st(n + 1), cs(n + 1);
    for (int64_t x = 0; x <= n; ++x) st[x] = x;
    for (int64_t i = 1; i <= m; ++i) {
        cur[0] = (int)i;
        cs[0] = 0;
        for (int64_t x = 1; x <= n; ++x) {
            const int a = row[x - 1] + (T[x - 1] != P[i - 1]), b = row[x] + 1, c = cur[x - 1] + 1;
            const int v = std::min(a, std::min(b, c));
            int64_t s = -1;
            if (a == v) s = std::max(s, st[x - 1]);
            if (b == v) s = std::max(s, st[x]);
            if (c == v) s = std::max(s, cs[x - 1]);
            cur[x] = v;
            cs[x] = s;
        }
        row.swap(cur);
        st.swap(cs);
    }
    D = row;
    best = st;
}

// ed(P, T[s, e)) for every s <= e by the anchored DP on the reversed strings: out[x] for s = e - x
static std::vector<int> anchored_back(const Str& T, const Str& P, uint64_t e) {
    const int64_t m = (int64_t)P.size, len = (int64_t)e;
    std::vector<int> row(len + 1), cur(len + 1);
    for (int64_t x = 0; x <= len; ++x) row[x] = (int)x;
    for (int64_t i = 1; i <= m; ++i) {
        cur[0] = (int)i;
        for (int64_t x = 1; x <= len; ++x)
            cur[x] = std::min(row[x - 1] + (T[e - x] != P[m - i]), std::min(row[x], cur[x - 1]) + 1);
        row.swap(cur);
    }
    return row;
}

// the definition of one band: diagonals c - k .. c + k, columns [0, n], row 0 zero inside, all else infinite
static uint64_t band_mask(const Str& T, const Str& P, int64_t k, int64_t c) {
    const int64_t n = (int64_t)T.size, m = (int64_t)P.size;
    auto inside = [&](int64_t i, int64_t x) { return x >= 0 && x <= n && x - i >= c - k && x - i <= c + k; };
    std::vector<int> row(n + 1, kInf), cur(n + 1);
    for (int64_t x = 0; x <= n; ++x)
        if (inside(0, x)) row[x] = 0;
    for (int64_t i = 1; i <= m; ++i) {
        for (int64_t x = 0; x <= n; ++x) {
            int v = kInf;
            if (inside(i, x)) {
                if (x > 0) v = std::min(v, row[x - 1] + (T[x - 1] != P[i - 1]));
                v = std::min(v, row[x] + 1);
                if (x > 0) v = std::min(v, cur[x - 1] + 1);
            }
            cur[x] = std::min(v, kInf);
        }
        row.swap(cur);
    }
    uint64_t mask = 0;
    for (int64_t t = 0; t <= 2 * k; ++t) {
        const int64_t x = c + m - k + t;
        if (x >= 0 && x <= n && row[x] <= k) mask |= 1ull << t;
    }
    return mask;
}

static bool check_band(const Str& T, const Str& P, uint32_t k, int64_t c) {
    const uint64_t want = band_mask(T, P, k, c);
    const uint64_t wide = sa::edit_verify_band<5>(T.size, P.size, k, c, T.words(), P.words());
    if (wide != want) FAIL("band n %llu m %llu k %u c %lld: %llx, not %llx", (ull)T.size, (ull)P.size, k, (long long)c, (ull)wide, (ull)want);
    if (k <= 3 && sa::edit_verify_band<2>(T.size, P.size, k, c, T.words(), P.words()) != want)
        FAIL("band (2 slices) n %llu m %llu k %u c %lld", (ull)T.size, (ull)P.size, k, (long long)c);
    ++g_checks;
    return true;
}

// one text, pattern and budget; all_diagonals: every diagonal that touches the text besides the seeds'
static bool check_case(const Str& T, const Str& P, uint32_t k, bool all_diagonals) {
    const uint64_t n = T.size, m = P.size;
    const Words tw = T.words(), pw = P.words();
    std::vector<int> D;
    std::vector<int64_t> best;
    sellers(T, P, D, best);
    std::vector<uint8_t> got(n + 1, 0);
    if (m <= k) {
        // not searched: no candidate gives an end
        for (uint32_t j = 0; j <= k; ++j)
            for (uint64_t h = 0; h < n + 2; ++h) {
                if (sa::edit_candidate_mask(n, m, k, j, h, tw, pw) != 0) FAIL("m %llu <= k %u gives an end", (ull)m, k);
                ++g_checks;
            }
        return true;
    }
    for (uint32_t j = 0; j <= k; ++j) {
        const uint64_t b = sa::ham_piece_bound(m, k, j), e = sa::ham_piece_bound(m, k, j + 1);
        if (e <= b) FAIL("piece %u of m %llu k %u is empty", j, (ull)m, k);
        for (uint64_t h = 0; h + (e - b) <= n; ++h) {
            bool hit = true;
            for (uint64_t t = 0; t < e - b && hit; ++t) hit = T[h + t] == P[b + t];
            if (!hit) continue;
            const uint64_t mask = sa::edit_candidate_mask(n, m, k, j, h, tw, pw);
            const int64_t c = (int64_t)h - (int64_t)b;
            const uint64_t band = band_mask(T, P, k, c);
            // the band's own answer, or nothing when an earlier piece matches on the diagonal
            if (mask != band) {
                bool earlier = false;
                for (uint32_t jj = 0; jj < j && !earlier && c >= 0; ++jj) {
                    const uint64_t bb = sa::ham_piece_bound(m, k, jj), ee = sa::ham_piece_bound(m, k, jj + 1);
                    bool same = (uint64_t)c + ee <= n;
                    for (uint64_t t = bb; t < ee && same; ++t) same = T[c + t] == P[t];
                    earlier = same;
                }
                if (mask != 0 || !earlier)
                    FAIL("candidate n %llu m %llu k %u j %u h %llu: %llx, band %llx", (ull)n, (ull)m, k, j, (ull)h, (ull)mask, (ull)band);
            }
            ++g_checks;
            for (uint32_t t = 0; t <= 2 * k; ++t)
                if ((mask >> t) & 1u) {
                    const uint64_t end = sa::edit_mask_end(m, k, j, h, t);
                    if (end > n) FAIL("end %llu of %llu", (ull)end, (ull)n);
                    got[end] = 1;
                }
            if (!check_band(T, P, k, c)) return false;
        }
        // a hit at or past n is no candidate
        for (uint64_t h : {n, n + 1, (uint64_t)0xFFFFFFFFull}) {
            if (sa::edit_candidate_mask(n, m, k, j, h, tw, pw) != 0) FAIL("a hit at %llu of %llu counts", (ull)h, (ull)n);
            ++g_checks;
        }
    }
    for (uint64_t e = 0; e <= n; ++e) {
        if ((D[e] <= (int)k) != (got[e] != 0))
            FAIL("n %llu m %llu k %u end %llu: D = %d, listed %d", (ull)n, (ull)m, k, (ull)e, D[e], (int)got[e]);
        ++g_checks;
        if (D[e] > (int)k) continue;
        uint64_t start = ~0ull;
        uint32_t dist = 999;
        if (!sa::edit_finish_end(m, k, e, tw, pw, start, dist)) FAIL("finish n %llu m %llu k %u end %llu: nothing", (ull)n, (ull)m, k, (ull)e);
        if ((int)dist != D[e]) FAIL("finish n %llu m %llu k %u end %llu: distance %u, not %d", (ull)n, (ull)m, k, (ull)e, dist, D[e]);
        if ((int64_t)start != best[e])
            FAIL("finish n %llu m %llu k %u end %llu: start %llu, not %lld", (ull)n, (ull)m, k, (ull)e, (ull)start, (long long)best[e]);
        g_checks += 2;
        if (all_diagonals) {   // the start by the definition itself: the smallest x with ed(P, T[e - x, e)) = D(e)
            const std::vector<int> back = anchored_back(T, P, e);
            uint64_t x = 0;
            while (back[x] != D[e]) ++x;
            if (*std::min_element(back.begin(), back.end()) != D[e] || e - x != start)
                FAIL("the definition's start n %llu m %llu k %u end %llu", (ull)n, (ull)m, k, (ull)e);
            ++g_checks;
        }
    }
    if (all_diagonals)
        for (int64_t c = -(int64_t)m - (int64_t)k - 2; c <= (int64_t)n + (int64_t)k + 2; ++c)
            if (!check_band(T, P, k, c)) return false;
    return true;
}

static std::vector<uint8_t> rand_str(std::mt19937_64& rng, uint64_t len, const std::vector<uint8_t>& sym) {
    std::vector<uint8_t> v(len);
    for (auto& c : v) c = sym[rng() % sym.size()];
    return v;
}

int main() {
    std::mt19937_64 rng(20240917);
    // the helpers
    for (int rep = 0; rep < 2000; ++rep) {
        const uint64_t w = rep < 4 ? (rep & 1 ? ~0ull : 0ull) : rng();
        const uint8_t b = rep < 4 ? (rep & 2 ? 0xFF : 0x00) : (uint8_t)(w >> (8 * (rng() % 8)));
        uint64_t want = 0, rev = 0;
        for (int j = 0; j < 8; ++j) want |= (uint64_t)(((w >> (8 * j)) & 0xFF) == b) << j;
        for (int j = 0; j < 64; ++j) rev |= ((w >> j) & 1ull) << (63 - j);
        if (sa::edit_eq_bytes(w, b) != want || sa::edit_reverse64(w) != rev) {
            std::printf("FAIL word helpers %llx %x\n", (ull)w, b);
            return 1;
        }
        ++g_checks;
    }
    // every text over {a, b} of up to 9 bytes against every pattern of up to 5, k <= 3
    for (uint64_t n = 0; n <= 9; ++n)
        for (uint64_t tb = 0; tb < (1ull << n); ++tb) {
            std::vector<uint8_t> t(n);
            for (uint64_t i = 0; i < n; ++i) t[i] = (tb >> i) & 1 ? 'b' : 'a';
            const Str T(t);
            for (uint64_t m = 0; m <= 5; ++m)
                for (uint64_t pb = 0; pb < (1ull << m); ++pb) {
                    std::vector<uint8_t> p(m);
                    for (uint64_t i = 0; i < m; ++i) p[i] = (pb >> i) & 1 ? 'b' : 'a';
                    const Str P(p);
                    for (uint32_t k = 0; k <= 3; ++k)
                        if (!check_case(T, P, k, n <= 5)) return 1;
                }
        }
    // random cases: 2 .. 4 symbols, 0x00 / 0xFF, patterns cut from the text with edits, m > n, m = k + 1, k = 31
    const std::vector<std::vector<uint8_t>> alphabets = {{'a', 'b'}, {'a', 'b', 'c'}, {'A', 'C', 'G', 'T'}, {0x00, 0xFF}};
    for (int rep = 0; rep < 2400; ++rep) {
        const auto& sym = alphabets[rep % alphabets.size()];
        const uint64_t n = rep % 7 == 0 ? 80 : 1 + rng() % 80;
        const std::vector<uint8_t> t = rand_str(rng, n, sym);
        uint32_t k = rep % 11 == 0 ? 31 : rep % 3 == 0 ? (uint32_t)(rng() % 32) : (uint32_t)(rng() % 5);
        uint64_t m = 1 + rng() % 70;
        if (rep % 5 == 1) m = k + 1;
        if (rep % 13 == 2) m = std::min<uint64_t>(70, n + 1 + rng() % (k + 2));   // m > n
        std::vector<uint8_t> p;
        if (rep % 4 != 3 && m <= n) {
            // a copy, at either end of the text every third time, with up to k + 1 edits
            const uint64_t at = rep % 3 == 0 ? 0 : rep % 3 == 1 ? n - m : rng() % (n - m + 1);
            p.assign(t.begin() + at, t.begin() + at + m);
            for (uint64_t s = rng() % (k + 2); s > 0; --s) {
                const uint64_t x = rng() % (p.size() + 1);
                const int kind = (int)(rng() % 3);
                if (kind == 0 && x < p.size()) p[x] = sym[rng() % sym.size()];
                else if (kind == 1 && x < p.size() && p.size() > 1) p.erase(p.begin() + x);
                else if (p.size() < 70) p.insert(p.begin() + x, sym[rng() % sym.size()]);
            }
        } else {
            p = rand_str(rng, m, sym);
        }
        if (!check_case(Str(t), Str(p), k, rep % 40 == 0)) return 1;
    }
    // the pinned answers of the contract
    {
        const Str T(std::vector<uint8_t>{'b', 'a', 'n', 'a', 'n', 'a'}), P(std::vector<uint8_t>{'a', 'n', 'a', 'n'});
        const uint64_t ends[] = {4, 5, 6}, starts[] = {1, 1, 3};
        const uint32_t dists[] = {1, 0, 1};
        for (int i = 0; i < 3; ++i) {
            uint64_t s = 99;
            uint32_t d = 99;
            if (!sa::edit_finish_end(4, 1, ends[i], T.words(), P.words(), s, d) || s != starts[i] || d != dists[i]) {
                std::printf("FAIL banana / anan end %llu\n", (ull)ends[i]);
                return 1;
            }
        }
        const Str abc(std::vector<uint8_t>{'a', 'b', 'c'}), abcd(std::vector<uint8_t>{'a', 'b', 'c', 'd'});
        if (!check_case(T, P, 1, true) || !check_case(abc, abcd, 1, true)) return 1;
        // m > n: piece 0 = "ab" at 0 finds the end 3
        if (sa::edit_candidate_mask(3, 4, 1, 0, 0, abc.words(), abcd.words()) != 1ull) {
            std::printf("FAIL abc / abcd\n");
            return 1;
        }
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
