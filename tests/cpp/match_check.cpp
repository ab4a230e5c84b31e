// Host check of the scalar longest-match search (sa::match_scalar,
// hpc_suffix_array_amd/csrc/sa_match.h) against a brute-force scan of the
// sorted suffixes: the longest prefix of P that occurs is found by comparing
// P with every suffix directly, its interval by counting the suffixes below
// and not above that prefix.  Random texts over 1, 2, 4 and 256 symbols,
// periodic texts, and synthetic accessors with no memory behind them at
// n = 2^32 - 1 (the only check of the 64-bit index arithmetic).  Every case
// runs with and without the bounds; the lengths must agree.  Text, SA and
// pattern live in exact-size heap buffers and are read bytewise, so a build
// with -fsanitize=address sees any read past either end.  Prints
// "ok <cases>" or the first mismatch.  Built by tests/test_match_core.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "sa_match.h"

typedef std::vector<uint8_t> Bytes;
typedef unsigned long long ull;

static long g_cases = 0;

// suffix at s against the first m bytes of p in the search's order: -1 below, 0 a prefix, 1 above
static int brute_cmp(const Bytes& t, uint64_t s, const Bytes& p, uint64_t m) {
    const uint64_t slen = t.size() - s, lim = std::min<uint64_t>(slen, m);
    const int c = lim ? std::memcmp(t.data() + s, p.data(), lim) : 0;
    if (c) return c < 0 ? -1 : 1;
    return slen >= m ? 0 : -1;
}

static std::vector<uint32_t> brute_sa(const Bytes& t) {
    const uint64_t n = t.size();
    std::vector<uint32_t> sa(n);
    for (uint64_t i = 0; i < n; ++i) sa[i] = (uint32_t)i;
    std::sort(sa.begin(), sa.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t la = n - a, lb = n - b;
        const int c = std::memcmp(t.data() + a, t.data() + b, std::min(la, lb));
        return c ? c < 0 : la < lb;
    });
    return sa;
}

static bool check(const Bytes& t, const std::vector<uint32_t>& sa, const Bytes& p, const char* what) {
    const uint64_t n = t.size(), m = p.size();
    uint64_t want_len = 0;
    for (uint64_t s = 0; s < n; ++s) {
        uint64_t k = 0;
        while (k < m && s + k < n && t[s + k] == p[k]) ++k;
        want_len = std::max(want_len, k);
    }
    uint64_t want_lo = 0, want_hi = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const int c = brute_cmp(t, sa[r], p, want_len);
        want_lo += c < 0;
        want_hi += c <= 0;
    }
    // exact-size heap copies, read bytewise: the sanitizer sees an over-read
    std::unique_ptr<uint8_t[]> tb(new uint8_t[n]), pb(new uint8_t[m]);
    std::unique_ptr<uint32_t[]> sb(new uint32_t[n]);
    std::copy(t.begin(), t.end(), tb.get());
    std::copy(p.begin(), p.end(), pb.get());
    std::copy(sa.begin(), sa.end(), sb.get());
    auto word = [](const uint8_t* b, uint64_t at, uint64_t end) {
        uint64_t x = 0;
        for (uint64_t i = at; i < end && i < at + 8; ++i) x |= (uint64_t)b[i] << (8 * (i - at));
        return x;
    };
    auto sa_at = [&](uint64_t r) { return sb[r]; };
    auto text_word = [&](uint64_t q) { return word(tb.get(), q, n); };
    auto pat_word = [&](uint64_t q) { return word(pb.get(), q, m); };
    uint64_t len = ~0ull, lo = ~0ull, hi = ~0ull, len_only = ~0ull, x = 0, y = 0;
    sa::match_scalar<true>(n, m, sa_at, text_word, pat_word, len, lo, hi);
    sa::match_scalar<false>(n, m, sa_at, text_word, pat_word, len_only, x, y);
    ++g_cases;
    if (len != want_len || lo != want_lo || hi != want_hi || len_only != want_len) {
        std::printf("mismatch (%s) n %llu m %llu: got %llu [%llu, %llu), lengths only %llu; want %llu [%llu, %llu)\n",
                    what, (ull)n, (ull)m, (ull)len, (ull)lo, (ull)hi, (ull)len_only, (ull)want_len, (ull)want_lo,
                    (ull)want_hi);
        return false;
    }
    if (len == m) {   // a full match: what sa_find gives
        uint64_t flo = ~0ull, fhi = ~0ull;
        sa::find_scalar(n, m, sa_at, text_word, pat_word, flo, fhi);
        if (flo != lo || fhi != hi) {
            std::printf("differs from find_scalar (%s) n %llu m %llu\n", what, (ull)n, (ull)m);
            return false;
        }
    }
    return true;
}

// both sides of the 8- and 16-byte words and of kFindEdge, the edge-probe threshold
static const uint64_t kLens[] = {0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 33, sa::kFindEdge - 1, sa::kFindEdge, sa::kFindEdge + 1};

static bool check_text(const Bytes& t, std::mt19937_64& rng, int cuts) {
    const uint64_t n = t.size();
    const std::vector<uint32_t> sa = brute_sa(t);
    auto sub = [&](uint64_t a, uint64_t len) { return Bytes(t.begin() + a, t.begin() + a + len); };
    for (int i = 0; i < cuts; ++i) {
        const uint64_t a = rng() % n;
        const uint64_t maxlen = n - a;
        uint64_t len = rng() % 4 ? kLens[rng() % (sizeof kLens / sizeof kLens[0])] : 1 + rng() % maxlen;
        len = std::min(len, maxlen);
        Bytes p = sub(a, len);
        if (!check(t, sa, p, "cut")) return false;                   // matches whole
        if (len == 0) continue;
        Bytes c = p;
        c[len - 1] = (uint8_t)(c[len - 1] + 1 + rng() % 255);
        if (!check(t, sa, c, "cut, last byte changed")) return false;
        c = p;
        c[0] ^= (uint8_t)(1 + rng() % 255);
        if (!check(t, sa, c, "cut, byte 0 changed")) return false;
        c = p;
        c[rng() % len] ^= (uint8_t)(1 + rng() % 255);
        if (!check(t, sa, c, "cut, one byte changed")) return false;
        c = p;
        for (int x : {0x00, 0x61, 0xFF}) c.push_back((uint8_t)x);
        if (!check(t, sa, c, "cut plus three bytes")) return false;
    }
    for (uint64_t tail : {(uint64_t)1, (uint64_t)5, (uint64_t)9, (uint64_t)17, (uint64_t)33, n}) {
        tail = std::min(tail, n);
        Bytes p = sub(n - tail, tail);
        if (!check(t, sa, p, "tail")) return false;
        for (int x : {0x00, 0x61, 0xFF}) {                           // runs past the text's end
            Bytes e = p;
            e.push_back((uint8_t)x);
            if (!check(t, sa, e, "tail plus a byte")) return false;
            e.resize(e.size() + 20, (uint8_t)x);
            if (!check(t, sa, e, "tail plus 21 bytes")) return false;
        }
    }
    if (!check(t, sa, Bytes(), "empty")) return false;
    for (uint64_t len : {(uint64_t)1, (uint64_t)8, (uint64_t)9, (uint64_t)40, n + 3}) {
        if (!check(t, sa, Bytes(len, 0x00), "all 0x00")) return false;
        if (!check(t, sa, Bytes(len, 0xFF), "all 0xFF")) return false;
    }
    return true;
}

// no memory: one symbol at n = 2^32 - 1, SA[r] = n - 1 - r; the pattern is
// a^j followed by m - j bytes `sym`
static bool check_synthetic() {
    const uint64_t n = 0xFFFFFFFFull;
    auto run = [&](uint64_t m, uint64_t j, uint8_t sym, uint64_t want_len, uint64_t want_lo, uint64_t want_hi) {
        auto text_word = [&](uint64_t at) {
            const uint64_t have = at < n ? std::min<uint64_t>(8, n - at) : 0;
            const uint64_t full = 0x0101010101010101ull * 'a';
            return have == 8 ? full : have == 0 ? 0 : full & ((1ull << (8 * have)) - 1);
        };
        auto pat_word = [&](uint64_t at) -> uint64_t {
            if (at + 8 <= j && at + 8 <= m) return 0x0101010101010101ull * 'a';
            uint64_t x = 0;
            for (uint64_t i = at; i < m && i < at + 8; ++i) x |= (uint64_t)(i < j ? 'a' : sym) << (8 * (i - at));
            return x;
        };
        auto sa_at = [&](uint64_t r) { return n - 1 - r; };
        uint64_t len = ~0ull, lo = ~0ull, hi = ~0ull, len_only = ~0ull, x = 0, y = 0;
        sa::match_scalar<true>(n, m, sa_at, text_word, pat_word, len, lo, hi);
        sa::match_scalar<false>(n, m, sa_at, text_word, pat_word, len_only, x, y);
        ++g_cases;
        if (len != want_len || lo != want_lo || hi != want_hi || len_only != want_len) {
            std::printf("synthetic mismatch m %llu j %llu sym %c: got %llu [%llu, %llu), lengths only %llu; want %llu "
                        "[%llu, %llu)\n", (ull)m, (ull)j, sym, (ull)len, (ull)lo, (ull)hi, (ull)len_only,
                        (ull)want_len, (ull)want_lo, (ull)want_hi);
            return false;
        }
        return true;
    };
    // a^k: k = n - 1 and n + 1 walk the whole text by words (about 10^9 steps a search)
    for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)17, (uint64_t)1000, n - 1, n + 1}) {
        const uint64_t len = std::min(k, n);
        if (!run(k, k, 'a', len, len - 1, n)) return false;
    }
    // a^j then a byte above / below 'a': the match is a^j, whose interval is [j - 1, n)
    for (uint64_t j : {(uint64_t)1, (uint64_t)8, (uint64_t)20, (uint64_t)1000}) {
        if (!run(j + 1, j, 'b', j, j - 1, n)) return false;
        if (!run(j + 1, j, 'A', j, j - 1, n)) return false;
        if (!run(j + 30, j, 'b', j, j - 1, n)) return false;
    }
    if (!run(1, 0, 'b', 0, 0, n)) return false;
    if (!run(1, 0, 'A', 0, 0, n)) return false;
    if (!run(40, 0, 'b', 0, 0, n)) return false;
    return run(0, 0, 'a', 0, 0, n);
}

int main() {
    std::mt19937_64 rng(20240611);
    for (int sigma : {1, 2, 4, 256}) {
        std::vector<uint64_t> sizes = {1, 2, 3, 7, 8, 9, 15, 16, 17, 18, 63, 64, 65, 1000, 3000};
        for (int i = 0; i < 5; ++i) sizes.push_back(1 + rng() % 3000);
        for (uint64_t n : sizes) {
            Bytes t(n);
            for (auto& b : t) b = sigma == 256 ? (uint8_t)rng() : (uint8_t)('a' + rng() % sigma);
            if (sigma == 256 && n > 4) t[rng() % n] = 0x00, t[rng() % n] = 0xFF;
            if (!check_text(t, rng, n > 100 ? 30 : 10)) return 1;
        }
    }
    // periodic: long shared prefixes on both sides of every probe
    for (uint64_t periods : {(uint64_t)3, (uint64_t)300}) {
        Bytes t;
        for (uint64_t i = 0; i < periods; ++i) t.insert(t.end(), {'a', 'b', 'a', 'a', 'b', 'a', 'b', 'a'});
        const std::vector<uint32_t> sa = brute_sa(t);
        for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)100, periods - 1, periods, periods + 1}) {
            if (k == 0 || k > periods + 1) continue;
            Bytes p;
            for (uint64_t i = 0; i < k; ++i) p.insert(p.end(), {'a', 'b', 'a', 'a', 'b', 'a', 'b', 'a'});
            if (!check(t, sa, p, "periods")) return 1;
            for (uint64_t cut : {(uint64_t)1, (uint64_t)5}) {
                Bytes s(p.begin() + cut, p.end());
                if (!check(t, sa, s, "periods, shifted")) return 1;
                s.resize(s.size() - 3);
                if (!check(t, sa, s, "periods, shifted and shortened")) return 1;
            }
            Bytes c = p;
            c[c.size() / 2] = 'c';
            if (!check(t, sa, c, "periods, middle byte raised")) return 1;
            c[c.size() / 2] = 'A';
            if (!check(t, sa, c, "periods, middle byte lowered")) return 1;
            c = p;
            c.back() = 'b';
            if (!check(t, sa, c, "periods, last byte changed")) return 1;
            c = p;
            c[0] = 'c';
            if (!check(t, sa, c, "periods, byte 0 changed")) return 1;
        }
        if (!check_text(t, rng, 30)) return 1;
    }
    if (!check_synthetic()) return 1;
    std::printf("ok %ld\n", g_cases);
    return 0;
}
