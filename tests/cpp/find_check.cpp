// Host check of the scalar pattern search (sa::find_scalar,
// hpc_suffix_array_amd/csrc/sa_find.h) against a brute-force scan of the
// sorted suffixes: random texts over 1, 2, 4 and 256 symbols (n = 1 .. 5000),
// periodic texts, and synthetic accessors with no memory behind them at
// n = 2^32 - 1 (the only check of the 64-bit index arithmetic).  Text and
// pattern live in exact-size heap buffers and are read bytewise, so a build
// with -fsanitize=address sees any read past either end.  Prints
// "ok <cases>" or the first mismatch.  Built by tests/test_find_core.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "sa_find.h"

typedef std::vector<uint8_t> Bytes;

static long g_cases = 0;

// suffix at s against P in the search's order: -1 below, 0 P is a prefix, 1 above
static int brute_cmp(const Bytes& t, uint64_t s, const Bytes& p) {
    const uint64_t slen = t.size() - s, lim = std::min<uint64_t>(slen, p.size());
    const int c = lim ? std::memcmp(t.data() + s, p.data(), lim) : 0;
    if (c) return c < 0 ? -1 : 1;
    return slen >= p.size() ? 0 : -1;
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
    uint64_t want_lo = 0, want_hi = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const int c = brute_cmp(t, sa[r], p);
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
    uint64_t lo = ~0ull, hi = ~0ull;
    sa::find_scalar(n, m, [&](uint64_t r) { return sb[r]; }, [&](uint64_t q) { return word(tb.get(), q, n); },
                    [&](uint64_t q) { return word(pb.get(), q, m); }, lo, hi);
    ++g_cases;
    if (lo != want_lo || hi != want_hi) {
        std::printf("mismatch (%s) n %llu m %llu: got [%llu, %llu) want [%llu, %llu)\n", what, (unsigned long long)n,
                    (unsigned long long)m, (unsigned long long)lo, (unsigned long long)hi,
                    (unsigned long long)want_lo, (unsigned long long)want_hi);
        return false;
    }
    return true;
}

static bool check_text(const Bytes& t, std::mt19937_64& rng, int cuts) {
    const uint64_t n = t.size();
    const std::vector<uint32_t> sa = brute_sa(t);
    auto sub = [&](uint64_t a, uint64_t len) { return Bytes(t.begin() + a, t.begin() + a + len); };
    for (int i = 0; i < cuts; ++i) {
        const uint64_t a = rng() % n;
        const uint64_t maxlen = n - a;
        // short lengths mostly (both sides of the 8- and 16-byte words), some long
        uint64_t len = 1 + (rng() % 4 ? rng() % 20 : rng() % maxlen);
        len = std::min(len, maxlen);
        Bytes p = sub(a, len);
        if (!check(t, sa, p, "cut")) return false;
        Bytes c = p;
        c[rng() % len] ^= (uint8_t)(1 + rng() % 255);
        if (!check(t, sa, c, "cut, one byte changed")) return false;
        c = p;
        c[len - 1] = (uint8_t)(c[len - 1] + 1);
        if (!check(t, sa, c, "cut, last byte + 1")) return false;
    }
    for (uint64_t tail : {(uint64_t)1, (uint64_t)5, (uint64_t)9, (uint64_t)17, n}) {
        tail = std::min(tail, n);
        Bytes p = sub(n - tail, tail);
        if (!check(t, sa, p, "tail")) return false;
        for (int x : {0x00, 0x61, 0xFF}) {
            Bytes e = p;
            e.push_back((uint8_t)x);
            if (!check(t, sa, e, "tail plus a byte")) return false;   // tail == n: the text plus a byte
        }
    }
    if (!check(t, sa, Bytes(), "empty")) return false;
    for (uint64_t len : {(uint64_t)1, (uint64_t)8, (uint64_t)9, (uint64_t)40, n + 3}) {
        if (!check(t, sa, Bytes(len, 0x00), "all 0x00")) return false;
        if (!check(t, sa, Bytes(len, 0xFF), "all 0xFF")) return false;
    }
    return true;
}

// no memory: one symbol at n = 2^32 - 1, SA[r] = n - 1 - r
static bool check_synthetic() {
    const uint64_t n = 0xFFFFFFFFull;
    auto run = [&](uint64_t m, uint8_t sym, uint64_t want_lo, uint64_t want_hi) {
        auto word = [](uint64_t at, uint64_t end, uint8_t s) {
            const uint64_t have = at < end ? std::min<uint64_t>(8, end - at) : 0;
            const uint64_t full = 0x0101010101010101ull * s;
            return have == 8 ? full : have == 0 ? 0 : full & ((1ull << (8 * have)) - 1);
        };
        uint64_t lo = ~0ull, hi = ~0ull;
        sa::find_scalar(n, m, [&](uint64_t r) { return n - 1 - r; }, [&](uint64_t q) { return word(q, n, 'a'); },
                        [&](uint64_t q) { return word(q, m, sym); }, lo, hi);
        ++g_cases;
        if (lo != want_lo || hi != want_hi) {
            std::printf("synthetic mismatch m %llu sym %c: got [%llu, %llu) want [%llu, %llu)\n",
                        (unsigned long long)m, sym, (unsigned long long)lo, (unsigned long long)hi,
                        (unsigned long long)want_lo, (unsigned long long)want_hi);
            return false;
        }
        return true;
    };
    // k = n - 1 and n walk the whole text twice by words (about 10^9 steps each)
    for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)1000, n - 1, n})
        if (!run(k, 'a', k - 1, n)) return false;
    if (!run(1, 'b', n, n)) return false;
    if (!run(1, 'A', 0, 0)) return false;
    return run(0, 'a', 0, n);
}

int main() {
    std::mt19937_64 rng(20240607);
    for (int sigma : {1, 2, 4, 256}) {
        std::vector<uint64_t> sizes = {1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 5000};
        for (int i = 0; i < 6; ++i) sizes.push_back(1 + rng() % 5000);
        for (uint64_t n : sizes) {
            Bytes t(n);
            for (auto& b : t) b = sigma == 256 ? (uint8_t)rng() : (uint8_t)('a' + rng() % sigma);
            if (sigma == 256 && n > 4) t[rng() % n] = 0x00, t[rng() % n] = 0xFF;
            if (!check_text(t, rng, n > 100 ? 40 : 12)) return 1;
        }
    }
    // periodic: long shared prefixes on both sides of every probe
    for (uint64_t periods : {(uint64_t)3, (uint64_t)500}) {
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
        }
        if (!check_text(t, rng, 30)) return 1;
    }
    if (!check_synthetic()) return 1;
    std::printf("ok %ld\n", g_cases);
    return 0;
}
