// Host check of the host-compilable core of the repeat enumeration
// (hpc_suffix_array_amd/csrc/sa_repeats.h): the nearest-smaller walks over a
// hierarchy of LCP minima built here on the host, with fan-out 64 and with
// fan-out 4 (three and more levels at these sizes), whole (one node a step and
// kLpfChunk nodes a step) and as the kernel composes them (a window of F * F
// ranks first, then the whole hierarchy from the window's edge, with the two
// shortcuts); the break-rank query over words of 64 ranks with 64, 2 and 1
// words per tile; the supermaximal scan.  All three kinds are compared, in
// head order, with the substring dictionary of the text: every substring with
// its occurrences, its followers (the end of the text is one) and its
// preceders (the start of the text is one); right-maximal = two occurrences
// and two followers, maximal = two preceders as well, supermaximal = maximal
// and no proper substring of another maximal repeat.
// The walks, the break rank and the scan at n = 2^32 - 1 run on accessors with
// no memory behind them.
// Every level and every break array is an exact-size heap allocation, so a
// build with -fsanitize=address sees any access past an end.  Prints
// "ok <checks> checks on <texts> texts" or the first mismatch.  Built by
// tests/test_repeats_core.py.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <random>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "sa_repeats.h"

typedef unsigned long long ull;
static long g_checks = 0;

#define FAIL(...)                         \
    do {                                  \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");                \
        return false;                     \
    } while (0)

template <class T>
struct Heap {   // exactly n entries
    std::unique_ptr<T[]> p;
    uint64_t n;
    explicit Heap(uint64_t n_) : p(new T[n_]), n(n_) {}
    T& operator[](uint64_t i) { return p[i]; }
    const T& operator[](uint64_t i) const { return p[i]; }
};

typedef std::array<uint64_t, 3> Triple;   // len, lo, hi

// the hierarchy of minima over ranks [lo, lo + len) of the LCP array; rank 0 reads as 0
template <uint32_t F>
struct Hier {
    std::vector<Heap<uint32_t>> lv;
    int n_levels = 0;
    mutable long reads = 0;
    Hier(const Heap<uint32_t>& l, uint64_t lo, uint64_t len, int force_levels = 0) {
        uint64_t cnt[sa::kLpfMaxLevels];
        n_levels = sa::lpf_level_counts<F>(len, cnt);
        if (force_levels)   // the kernel's window: always three levels
            for (; n_levels < force_levels; ++n_levels) cnt[n_levels] = 1;
        for (int k = 0; k < n_levels; ++k) lv.emplace_back(cnt[k]);
        for (uint64_t i = 0; i < len; ++i) lv[0][i] = lo + i == 0 ? 0u : l[lo + i];
        for (int k = 1; k < n_levels; ++k)
            for (uint64_t p = 0; p < lv[k].n; ++p) {
                uint32_t m = ~0u;
                for (uint64_t c = p * F; c < std::min<uint64_t>(p * F + F, lv[k - 1].n); ++c) m = std::min(m, lv[k - 1][c]);
                lv[k][p] = m;
            }
    }
    int levels() const { return n_levels; }
    uint64_t count(int k) const { return lv[k].n; }
    uint32_t operator()(int k, uint64_t i) const {
        ++reads;
        if (k < 0 || k >= n_levels || i >= lv[k].n) {
            std::printf("FAIL node (%d, %llu) read\n", k, (ull)i);
            std::abort();
        }
        return lv[k][i];
    }
};

// the break bits of a text: words of 64 ranks, WPT words per tile
struct Breaks {
    Heap<uint64_t> words;
    Heap<uint32_t> cnt;
    Heap<uint64_t> tiles;
    Breaks(const Heap<uint32_t>& prev, uint64_t n, uint32_t wpt)
        : words((n + 63) / 64), cnt((n + 63) / 64), tiles(((n + 63) / 64 + wpt - 1) / wpt) {
        for (uint64_t w = 0; w < words.n; ++w) {
            uint64_t m = 0;
            for (uint64_t k = 0; k < 64 && w * 64 + k < n; ++k) {
                const uint64_t r = w * 64 + k;
                if (r > 0 && prev[r] != prev[r - 1]) m |= 1ull << k;
            }
            words[w] = m;
        }
        uint64_t total = 0;
        for (uint64_t t = 0; t < tiles.n; ++t) {
            tiles[t] = total;
            uint32_t in_tile = 0;
            for (uint64_t w = t * wpt; w < std::min<uint64_t>(t * wpt + wpt, words.n); ++w) {
                cnt[w] = in_tile;
                in_tile += (uint32_t)__builtin_popcountll(words[w]);
            }
            total += in_tile;
        }
    }
    uint64_t word(uint64_t w) const { return at(words, w, "word"); }
    uint64_t count(uint64_t w) const { return at(cnt, w, "count"); }
    uint64_t tile(uint64_t t) const { return at(tiles, t, "tile"); }
    template <class T>
    static uint64_t at(const Heap<T>& h, uint64_t i, const char* what) {
        if (i >= h.n) {
            std::printf("FAIL break %s %llu read\n", what, (ull)i);
            std::abort();
        }
        return h[i];
    }
};

static std::vector<uint8_t> make_text(int kind, uint64_t n, std::mt19937& rng) {
    std::vector<uint8_t> t(n);
    for (uint64_t i = 0; i < n; ++i) {
        switch (kind) {
        case 0: t[i] = "ACGT"[rng() & 3]; break;
        case 1: t[i] = (rng() & 1) ? 0x00 : 0xFF; break;
        case 2: t[i] = (uint8_t)rng(); break;
        case 3: t[i] = 'a'; break;
        case 4: t[i] = i + 1 == n ? 'b' : 'a'; break;
        case 5: t[i] = i == 0 ? 'b' : 'a'; break;
        case 6: t[i] = i % 7 == 6 ? 'b' : 'a'; break;   // (a^6 b)^j: a sawtooth SA
        case 7: t[i] = "abc"[i % 3]; break;
        case 8: t[i] = (uint8_t)(i < n / 2 ? rng() % 3 : 0); break;
        default: t[i] = (uint8_t)(255 - i % 256); break;
        }
    }
    if (kind == 8)   // R + R
        for (uint64_t i = n / 2; i < n; ++i) t[i] = t[i - n / 2];
    return t;
}

// "ab", then c "ab" for every byte c: ab occurs 257 times with pairwise
// distinct followers (the end included) and preceders (the start included)
static std::vector<uint8_t> sup257() {
    std::vector<uint8_t> t = {'a', 'b'};
    for (int c = 0; c < 256; ++c) {
        t.push_back((uint8_t)c);
        t.push_back('a');
        t.push_back('b');
    }
    return t;
}

static uint64_t common(const std::vector<uint8_t>& t, uint64_t a, uint64_t b) {
    uint64_t k = 0;
    while (a + k < t.size() && b + k < t.size() && t[a + k] == t[b + k]) ++k;
    return k;
}

struct Entry {
    uint64_t count = 0, min_rank = ~0ull;
    uint64_t fol[5] = {0, 0, 0, 0, 0}, pre[5] = {0, 0, 0, 0, 0};   // 257 symbols
    static void set(uint64_t (&m)[5], uint32_t c) { m[c >> 6] |= 1ull << (c & 63); }
    static int size(const uint64_t (&m)[5]) {
        int k = 0;
        for (uint64_t x : m) k += __builtin_popcountll(x);
        return k;
    }
};

// the three kinds by the substring dictionary, each sorted by head
static bool by_dictionary(const std::vector<uint8_t>& t, const Heap<uint32_t>& rank, const Heap<uint32_t>& l,
                          std::vector<Triple> (&want)[3]) {
    const uint64_t n = t.size();
    uint64_t longest = 0;   // a longer substring occurs once
    for (uint64_t r = 1; r < n; ++r) longest = std::max<uint64_t>(longest, l[r]);
    const char* base = (const char*)t.data();
    std::unordered_map<std::string_view, Entry> dict;
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t len = 1; len <= longest && i + len <= n; ++len) {
            Entry& e = dict[std::string_view(base + i, len)];
            ++e.count;
            e.min_rank = std::min<uint64_t>(e.min_rank, rank[i]);
            Entry::set(e.fol, i + len < n ? t[i + len] : 256u);
            Entry::set(e.pre, i > 0 ? t[i - 1] : 256u);
        }
    // every proper substring of a maximal repeat: drop a first or a last byte, again and again
    std::unordered_set<std::string_view> inside;
    std::deque<std::string_view> todo;
    for (const auto& kv : dict)
        if (kv.second.count >= 2 && Entry::size(kv.second.fol) >= 2 && Entry::size(kv.second.pre) >= 2)
            todo.push_back(kv.first);
    while (!todo.empty()) {
        const std::string_view w = todo.front();
        todo.pop_front();
        if (w.size() < 2) continue;
        for (const std::string_view s : {w.substr(1), w.substr(0, w.size() - 1)})
            if (inside.insert(s).second) todo.push_back(s);
    }
    std::vector<std::array<uint64_t, 4>> rows[3];   // head first
    for (const auto& kv : dict) {
        const Entry& e = kv.second;
        if (e.count < 2 || Entry::size(e.fol) < 2) continue;
        const uint64_t len = kv.first.size(), lo = e.min_rank, hi = lo + e.count;
        uint64_t head = 0;
        for (uint64_t k = lo + 1; k < hi && !head; ++k)
            if (l[k] == len) head = k;
        if (!head) FAIL("n=%llu: the right-maximal substring of length %llu at rank %llu has no head", (ull)n, (ull)len, (ull)lo);
        rows[0].push_back({head, len, lo, hi});
        if (Entry::size(e.pre) < 2) continue;
        rows[1].push_back({head, len, lo, hi});
        if (!inside.count(kv.first)) rows[2].push_back({head, len, lo, hi});
    }
    for (int kind = 0; kind < 3; ++kind) {
        std::sort(rows[kind].begin(), rows[kind].end());
        want[kind].clear();
        for (const auto& r : rows[kind]) want[kind].push_back({r[1], r[2], r[3]});
        for (size_t k = 1; k < rows[kind].size(); ++k)
            if (rows[kind][k][0] == rows[kind][k - 1][0]) FAIL("n=%llu: rank %llu heads two repeats", (ull)n, (ull)rows[kind][k][0]);
    }
    return true;
}

template <uint32_t F>
static bool check_walks(const std::vector<uint8_t>& t, const Heap<uint32_t>& s, const Heap<uint32_t>& l,
                        const Heap<uint32_t>& prev, const std::vector<Triple> (&want)[3]) {
    const uint64_t n = t.size();
    if (n == 0) return want[0].empty();
    const Hier<F> g(l, 0, n);
    const Breaks b64(prev, n, 64), b2(prev, n, 2), b1(prev, n, 1);
    const auto lcp_at = [&](uint64_t r) -> uint32_t {
        if (r == 0 || r >= n) {
            std::printf("FAIL lcp[%llu] read by the scan\n", (ull)r);
            std::abort();
        }
        return l[r];
    };
    long scanned = 0;
    const auto prev_at = [&](uint64_t r) -> uint32_t {
        if (r >= n) {
            std::printf("FAIL prev(%llu) read\n", (ull)r);
            std::abort();
        }
        ++scanned;
        return prev[r];
    };
    std::vector<Triple> got[3];
    const uint64_t W = (uint64_t)F * F;
    for (uint64_t base = 0; base < n; base += W) {
        const uint64_t len = std::min<uint64_t>(W, n - base);
        const Hier<F> win(l, base, len, 3);
        for (uint64_t r = std::max<uint64_t>(base, 1); r < base + len; ++r) {
            const uint32_t v = l[r];
            if (v == 0) continue;
            const uint32_t before = r == 1 ? 0u : l[r - 1];
            // whole, one node a step: the nearest entry <= v to the left, the nearest < v to the right
            uint64_t j = 0, lo1 = 0, hi1 = n, lo2 = 0;
            g.reads = 0;
            if (!sa::rep_walk_left<true, F, 1>(g, r, v, j)) FAIL("F=%u n=%llu rank %llu: nothing <= %u to its left", F, (ull)n, (ull)r, v);
            const bool head1 = g(0, j) < v;
            lo1 = j;
            if (sa::rep_walk_right<false, F, 1>(g, r, v, j)) hi1 = j;
            if (g.reads > 2L * 2 * F * g.levels())
                FAIL("F=%u n=%llu rank %llu: %ld reads for %d levels", F, (ull)n, (ull)r, g.reads, g.levels());
            // the definition of both
            uint64_t a = r - 1;
            while (a > 0 && l[a] > v) --a;
            uint64_t e = r + 1;
            while (e < n && l[e] >= v) ++e;
            if (lo1 != a || hi1 != e || head1 != ((a == 0 ? 0u : l[a]) < v))
                FAIL("F=%u n=%llu rank %llu: walks give [%llu, %llu), the scan [%llu, %llu)", F, (ull)n, (ull)r, (ull)lo1,
                     (ull)hi1, (ull)a, (ull)e);
            // kLpfChunk nodes a step
            uint64_t hi2 = n;
            if (!sa::rep_walk_left<true, F, sa::kLpfChunk>(g, r, v, lo2) || lo2 != lo1) FAIL("F=%u n=%llu rank %llu: chunked left walk", F, (ull)n, (ull)r);
            if (sa::rep_walk_right<false, F, sa::kLpfChunk>(g, r, v, j)) hi2 = j;
            if (hi2 != hi1) FAIL("F=%u n=%llu rank %llu: chunked right walk", F, (ull)n, (ull)r);
            // the window, then the whole from its edge, with the shortcuts
            uint64_t lo3 = 0;
            const bool head3 = sa::rep_head_lo<F>(win, g, base, r - base, v, before, lo3);
            if (head3 != head1 || (head3 && lo3 != lo1)) FAIL("F=%u n=%llu rank %llu: window walk gives lo %llu (head %d), the whole %llu (head %d)", F, (ull)n, (ull)r, (ull)lo3, (int)head3, (ull)lo1, (int)head1);
            g_checks += 3;
            if (!head3) continue;
            const uint64_t hi3 = sa::rep_head_hi<F>(win, g, base, r - base, v, n);
            if (hi3 != hi1) FAIL("F=%u n=%llu rank %llu: window walk gives hi %llu, the whole %llu", F, (ull)n, (ull)r, (ull)hi3, (ull)hi1);
            got[0].push_back({v, lo3, hi3});
            const bool lm = sa::rep_left_maximal<64>(b64, lo3, hi3);
            if (lm != sa::rep_left_maximal<2>(b2, lo3, hi3) || lm != sa::rep_left_maximal<1>(b1, lo3, hi3))
                FAIL("F=%u n=%llu rank %llu: the break rank depends on the tile size", F, (ull)n, (ull)r);
            bool differ = false;
            for (uint64_t k = lo3 + 1; k < hi3; ++k) differ = differ || prev[k] != prev[lo3];
            if (lm != differ) FAIL("F=%u n=%llu rank %llu: left-maximal %d, by the symbols %d", F, (ull)n, (ull)r, (int)lm, (int)differ);
            if (lm) got[1].push_back({v, lo3, hi3});
            uint64_t hs = 0;
            scanned = 0;
            if (before < v && sa::rep_supermaximal(lcp_at, prev_at, n, r, v, hs)) {
                if (hs != hi3 || hs - lo3 > (uint64_t)sa::kRepSuperMax) FAIL("F=%u n=%llu rank %llu: the scan ends at %llu, the walk at %llu", F, (ull)n, (ull)r, (ull)hs, (ull)hi3);
                got[2].push_back({v, lo3, hi3});
            }
            if (scanned > sa::kRepSuperMax) FAIL("F=%u n=%llu rank %llu: the scan read %ld ranks", F, (ull)n, (ull)r, scanned);
            g_checks += 3;
        }
    }
    for (int kind = 0; kind < 3; ++kind) {
        if (got[kind] != want[kind]) {
            size_t k = 0;
            while (k < got[kind].size() && k < want[kind].size() && got[kind][k] == want[kind][k]) ++k;
            FAIL("F=%u n=%llu kind %d: %zu repeats, the dictionary has %zu; they differ at %zu", F, (ull)n, kind,
                 got[kind].size(), want[kind].size(), k);
        }
        g_checks += (long)want[kind].size() + 1;
    }
    (void)s;
    return true;
}

static bool check_text(const std::vector<uint8_t>& t) {
    const uint64_t n = t.size();
    Heap<uint32_t> s(n), l(n), rank(n), prev(n);
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t k = common(t, a, b);
        if (a + k == n || b + k == n) return a > b;   // the shorter suffix (the larger position) first
        return t[a + k] < t[b + k];
    });
    for (uint64_t r = 0; r < n; ++r) {
        s[r] = order[r];
        rank[order[r]] = (uint32_t)r;
        l[r] = r ? (uint32_t)common(t, order[r - 1], order[r]) : 0u;
        prev[r] = order[r] ? (uint32_t)t[order[r] - 1] : sa::kRepStart;
    }
    std::vector<Triple> want[3];
    if (!by_dictionary(t, rank, l, want)) return false;
    // the kinds are nested
    if (want[2].size() > want[1].size() || want[1].size() > want[0].size()) FAIL("n=%llu: the kinds are not nested", (ull)n);
    return check_walks<64>(t, s, l, prev, want) && check_walks<4>(t, s, l, prev, want);
}

// n = 2^32 - 1 with nothing behind the accessors: lcp[0] = 0, every other entry 1
struct Flat {
    uint64_t cnt[sa::kLpfMaxLevels];
    int n_levels;
    mutable long reads = 0;
    int levels() const { return n_levels; }
    uint64_t count(int k) const { return cnt[k]; }
    uint32_t operator()(int k, uint64_t i) const {
        ++reads;
        if (k < 0 || k >= n_levels || i >= cnt[k]) {
            std::printf("FAIL node (%d, %llu) read\n", k, (ull)i);
            std::abort();
        }
        return i == 0 ? 0u : 1u;
    }
};

struct AllBreaks {   // every rank is a break
    uint64_t n;
    uint64_t word(uint64_t w) const { return chk(w, (n + 63) / 64), ~0ull; }
    uint64_t count(uint64_t w) const { return chk(w, (n + 63) / 64), (w % 64) * 64; }
    uint64_t tile(uint64_t t) const { return chk(t, (n + 4095) / 4096), t * 4096; }
    static void chk(uint64_t i, uint64_t end) {
        if (i >= end) {
            std::printf("FAIL break entry %llu read\n", (ull)i);
            std::abort();
        }
    }
};

static bool check_large() {
    const uint64_t n = 0xFFFFFFFFull;
    Flat h;
    h.n_levels = sa::lpf_level_counts<64>(n, h.cnt);
    if (h.n_levels != 7 || h.cnt[1] != (1ull << 26) || h.cnt[6] != 1) FAIL("level counts at 2^32 - 1");
    // the level counts as the kernels compute them
    for (uint64_t m : {(uint64_t)1, (uint64_t)2, (uint64_t)63, (uint64_t)64, (uint64_t)65, (uint64_t)4096, (uint64_t)4097,
                       (uint64_t)262143, (uint64_t)262144, (uint64_t)262145, (uint64_t)1 << 24, ((uint64_t)1 << 24) + 1, n - 1, n}) {
        uint64_t cnt[sa::kLpfMaxLevels];
        const int levels = sa::lpf_level_counts<64>(m, cnt);
        for (int k = 0; k < levels; ++k)
            if (sa::rep_level_count(m, k) != cnt[k]) FAIL("level %d of %llu entries: %llu nodes, not %llu", k, (ull)m, (ull)sa::rep_level_count(m, k), (ull)cnt[k]);
        g_checks += levels;
    }
    const long bound = (64 + sa::kLpfChunk) * 2 * 7;
    for (uint64_t r : {(uint64_t)1, (uint64_t)5, (uint64_t)4095, (uint64_t)4096, (uint64_t)123456789, n - 2, n - 1}) {
        uint64_t j = 0;
        h.reads = 0;
        if (!sa::rep_walk_left<true, 64, sa::kLpfChunk>(h, r, 1u, j) || j != r - 1 || h.reads > bound) FAIL("flat LCP: <= 1 to the left of %llu", (ull)r);
        h.reads = 0;
        if (!sa::rep_walk_left<true, 64, sa::kLpfChunk>(h, r, 0u, j) || j != 0 || h.reads > bound) FAIL("flat LCP: the walk to rank 0 from %llu (%ld reads)", (ull)r, h.reads);
        h.reads = 0;
        if (sa::rep_walk_left<false, 64, sa::kLpfChunk>(h, r, 0u, j) || h.reads > bound) FAIL("flat LCP: something < 0 to the left of %llu", (ull)r);
        h.reads = 0;
        if (sa::rep_walk_right<false, 64, sa::kLpfChunk>(h, r, 1u, j) || h.reads > bound) FAIL("flat LCP: something < 1 to the right of %llu (%ld reads)", (ull)r, h.reads);
        h.reads = 0;
        const bool f = sa::rep_walk_right<true, 64, sa::kLpfChunk>(h, r, 1u, j);
        if (f != (r + 1 < n) || (f && j != r + 1)) FAIL("flat LCP: <= 1 to the right of %llu", (ull)r);
        // the kernel's composition in the last tile: a window of the tile, the whole from its edges
        const uint64_t base = r / 4096 * 4096;
        struct Win {
            uint64_t c0;
            uint64_t base;
            int levels() const { return 3; }
            uint64_t count(int k) const { return k == 0 ? c0 : k == 1 ? (c0 + 63) / 64 : 1; }
            uint32_t operator()(int k, uint64_t i) const {
                if (i >= count(k)) {
                    std::printf("FAIL window node (%d, %llu) read\n", k, (ull)i);
                    std::abort();
                }
                return base == 0 && i == 0 ? 0u : 1u;
            }
        } win{std::min<uint64_t>(4096, n - base), base};
        uint64_t lo = 0;
        if (sa::rep_head_lo<64>(win, h, base, r - base, 1u, r == 1 ? 0u : 1u, lo) != (r == 1) || (r == 1 && lo != 0)) FAIL("flat LCP: head at %llu", (ull)r);
        if (sa::rep_head_hi<64>(win, h, base, r - base, 1u, n) != n) FAIL("flat LCP: the interval of %llu ends before n", (ull)r);
        // a descent (as if the rank below held 2): the entry found is 1, no head, but for rank 0's 0
        if (sa::rep_head_lo<64>(win, h, base, r - base, 1u, 2u, lo) != (r == 1) || (r == 1 && lo != 0)) FAIL("flat LCP: descent at %llu", (ull)r);
        g_checks += 8;
    }
    const AllBreaks b{n};
    if (sa::rep_break_rank<64>(b, n - 1) != n || sa::rep_break_rank<64>(b, 0) != 1 || sa::rep_break_rank<64>(b, 4095) != 4096 ||
        sa::rep_break_rank<64>(b, 4096) != 4097 || sa::rep_break_rank<64>(b, 63) != 64 || sa::rep_break_rank<64>(b, 64) != 65 ||
        !sa::rep_left_maximal<64>(b, n - 3, n) || !sa::rep_left_maximal<64>(b, 0, n))
        FAIL("break ranks at n = 2^32 - 1");
    g_checks += 8;
    // the scan: 101 distinct symbols up to the last rank; 257 distinct ones and a 258th occurrence
    long reads = 0;
    uint64_t k = n - 100, hi = 0;
    const auto lcp5 = [&](uint64_t r) -> uint32_t {
        if (r <= k || r >= n) {
            std::printf("FAIL lcp[%llu] read\n", (ull)r);
            std::abort();
        }
        return 5u;
    };
    const auto prev_k = [&](uint64_t r) -> uint32_t {
        ++reads;
        if (r + 1 < k || r >= n) {
            std::printf("FAIL prev(%llu) read\n", (ull)r);
            std::abort();
        }
        return (uint32_t)((r - (k - 1)) % 257);   // 256: the start
    };
    if (!sa::rep_supermaximal(lcp5, prev_k, n, k, 5u, hi) || hi != n || reads != 101) FAIL("the scan up to rank n - 1");
    k = n - 256;   // ranks k - 1 .. n - 1: 257 occurrences, all symbols once
    reads = 0;
    if (!sa::rep_supermaximal(lcp5, prev_k, n, k, 5u, hi) || hi != n || reads != 257) FAIL("the scan over 257 occurrences");
    k = n - 1000;  // the plateau goes on: the scan gives up after 257 ranks
    reads = 0;
    if (sa::rep_supermaximal(lcp5, prev_k, n, k, 5u, hi) || reads > 257) FAIL("the scan over a longer plateau (%ld reads)", reads);
    k = n - 257;   // 258 occurrences
    reads = 0;
    if (sa::rep_supermaximal(lcp5, prev_k, n, k, 5u, hi) || reads > 257) FAIL("the scan over 258 occurrences (%ld reads)", reads);
    g_checks += 4;
    if (sa::rep_min_len(0) != 1 || sa::rep_min_len(1) != 1 || sa::rep_min_len(7) != 7 || sa::rep_min_occ(0) != 2 ||
        sa::rep_min_occ(1) != 2 || sa::rep_min_occ(2) != 2 || sa::rep_min_occ(300) != 300)
        FAIL("the filters' defaults");
    g_checks += 7;
    return true;
}

int main() {
    std::mt19937 rng(12345);
    const uint64_t sizes[] = {0, 1, 2, 3, 4, 5, 7, 15, 16, 17, 31, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300};
    int texts = 0;
    for (int kind = 0; kind < 10; ++kind)
        for (uint64_t n : sizes) {
            if (!check_text(make_text(kind, n, rng))) return 1;
            ++texts;
        }
    for (int rep = 0; rep < 80; ++rep) {   // more random ones at random sizes
        if (!check_text(make_text(rep % 3, rng() % 301, rng))) return 1;
        ++texts;
    }
    // the largest supermaximal repeat, and one occurrence more: maximal, not supermaximal
    {
        std::vector<uint8_t> t = sup257();
        if (!check_text(t)) return 1;
        std::vector<uint8_t> u = t;
        u.push_back(7);
        u.push_back('a');
        u.push_back('b');
        if (!check_text(u)) return 1;
        // in front of them, filler over other bytes: the interval of "ab" moves up the ranks
        for (const std::vector<uint8_t>& x : {t, u}) {
            std::vector<uint8_t> f(40);
            for (size_t i = 0; i < f.size(); ++i) f[i] = (uint8_t)(i % 3);   // bytes 0, 1, 2 sort below 'a'
            f.insert(f.end(), x.begin(), x.end());
            if (!check_text(f)) return 1;
        }
        texts += 4;
    }
    if (!check_large()) return 1;
    std::printf("ok %ld checks on %d texts\n", g_checks, texts);
    return 0;
}
