// Host check of the arithmetic of the batched locate (hpc_suffix_array_amd/
// csrc/sa_locate.h) against brute force: the capped count and the class, the
// queries and slots of an output tile (random offset arrays with runs of empty
// queries and with large queries; every small query in exactly one tile, a
// tile below 2 * kLocateTile hits), the same on accessors with no memory
// behind them (offsets above 2^32, nq = 2^32 - 1), the composite key of the
// large class and the split of an output range for 16-byte stores.  The
// offset arrays are exact-size heap buffers, so a build with
// -fsanitize=address sees any read past either end.  Prints "ok <cases>" or
// the first mismatch.  Built by tests/test_locate_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "sa_locate.h"

typedef unsigned long long ull;
static const uint64_t T = sa::kLocateTile;
static long g_cases = 0;

#define FAIL(...)                      \
    do {                               \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");             \
        return false;                  \
    } while (0)

struct VecOff {
    const uint64_t* p;
    uint64_t size;   // nq + 1
    uint64_t operator()(uint64_t i) const {
        if (i >= size) {
            std::printf("FAIL offset %llu read of %llu\n", (ull)i, (ull)size);
            std::abort();
        }
        return p[i];
    }
};

static bool check_counts() {
    const uint64_t counts[] = {0, 1, T - 1, T, T + 1};
    const uint64_t caps[] = {0, 1, T, T + 1};
    const uint64_t n = 5 * T;
    for (uint64_t c : counts)
        for (uint64_t cap : caps)
            for (uint64_t lo : {(uint64_t)0, (uint64_t)7, n - c}) {
                const uint64_t want = cap ? std::min(c, cap) : c;
                const uint32_t got = sa::locate_count(lo, lo + c, n, cap);
                if (got != want) FAIL("count %llu cap %llu: %u", (ull)c, (ull)cap, got);
                if (sa::locate_large(got) != (want > T)) FAIL("class of %llu cap %llu", (ull)c, (ull)cap);
                ++g_cases;
            }
    // intervals that break lo <= hi <= n are empty; the widest valid one is whole
    if (sa::locate_count(5, 4, 10, 0) || sa::locate_count(0, 11, 10, 0) || sa::locate_count(11, 12, 10, 0) ||
        sa::locate_count(0xFFFFFFFFull, 0, 0xFFFFFFFFull, 0))
        FAIL("an invalid interval is not empty");
    if (sa::locate_count(0, 0xFFFFFFFFull, 0xFFFFFFFFull, 0) != 0xFFFFFFFFu) FAIL("whole SA at n = 2^32 - 1");
    if (sa::locate_count(0, 0xFFFFFFFFull, 0xFFFFFFFFull, 1ull << 40) != 0xFFFFFFFFu) FAIL("cap above 2^32");
    g_cases += 6;
    return true;
}

// every tile of an explicit offset array against a linear scan
static bool check_tiles(const std::vector<uint64_t>& cnt, const char* what) {
    const uint64_t nq = cnt.size();
    std::vector<uint64_t> offv(nq + 1, 0);
    for (uint64_t q = 0; q < nq; ++q) offv[q + 1] = offv[q] + cnt[q];
    // exact-size heap copy
    std::unique_ptr<uint64_t[]> heap(new uint64_t[nq + 1]);
    std::copy(offv.begin(), offv.end(), heap.get());
    const VecOff off{heap.get(), nq + 1};
    const uint64_t total = offv[nq], tiles = (total + T - 1) / T;
    std::vector<int> seen(nq, 0);
    for (uint64_t t = 0; t <= tiles; ++t) {   // one tile past the end too: it is empty
        uint64_t first = nq;
        for (uint64_t q = 0; q < nq; ++q)
            if (offv[q] >= t * T) {
                first = q;
                break;
            }
        if (sa::locate_tile_first(off, nq, t) != first)
            FAIL("%s: tile %llu first query %llu, want %llu", what, (ull)t, (ull)sa::locate_tile_first(off, nq, t),
                 (ull)first);
        const sa::LocateTile r = sa::locate_tile(off, nq, t);
        if (r.q0 != first || r.q1 < r.q0 || r.q1 > nq || r.s != offv[r.q0] || r.e != offv[r.q1])
            FAIL("%s: tile %llu range", what, (ull)t);
        if (r.e - r.s >= 2 * T) FAIL("%s: tile %llu holds %llu hits", what, (ull)t, (ull)(r.e - r.s));
        if (t == tiles && r.e != r.s) FAIL("%s: a tile past the end holds hits", what);
        for (uint64_t q = r.q0; q < r.q1; ++q) {
            if (cnt[q] == 0) continue;
            if (cnt[q] > T) FAIL("%s: tile %llu holds large query %llu", what, (ull)t, (ull)q);
            if (offv[q] / T != t) FAIL("%s: query %llu in tile %llu", what, (ull)q, (ull)t);
            ++seen[q];
        }
        ++g_cases;
    }
    for (uint64_t q = 0; q < nq; ++q)
        if (seen[q] != (cnt[q] > 0 && cnt[q] <= T ? 1 : 0))
            FAIL("%s: query %llu (%llu hits) in %d tiles", what, (ull)q, (ull)cnt[q], seen[q]);
    return true;
}

static bool check_random_tiles() {
    std::mt19937_64 rng(12345);
    for (int round = 0; round < 300; ++round) {
        const uint64_t nq = 1 + rng() % 400;
        std::vector<uint64_t> cnt(nq);
        const int kind = round % 6;
        for (uint64_t q = 0; q < nq;) {
            uint64_t c;
            switch (kind) {
                case 0: c = rng() % 4; break;                                   // tiny
                case 1: c = rng() % (T + 1); break;                             // any small
                case 2: c = (rng() % 8 == 0) ? T + 1 + rng() % (3 * T) : rng() % 64; break;   // some large
                case 3: c = (rng() % 3 == 0) ? T - 1 + rng() % 3 : rng() % 3; break;          // around the class boundary
                case 4: c = 1; break;
                default: c = (rng() % 4 == 0) ? T : T - 1 + rng() % 2; break;
            }
            cnt[q++] = c;
            if (rng() % 5 == 0)   // a run of empty queries
                for (uint64_t e = rng() % 40; e && q < nq; --e) cnt[q++] = 0;
        }
        char what[32];
        std::snprintf(what, sizeof what, "random %d", round);
        if (!check_tiles(cnt, what)) return false;
    }
    // the shapes the GPU test packs
    std::vector<uint64_t> a(T - 1, 1);
    a.push_back(T);   // a T-hit query on the last slot of tile 0: 2T - 1 hits
    if (!check_tiles(a, "2T - 1")) return false;
    if (!check_tiles(std::vector<uint64_t>(7, T), "exact tiles")) return false;
    if (!check_tiles(std::vector<uint64_t>(3 * T + 1, 1), "one-hit queries")) return false;
    if (!check_tiles(std::vector<uint64_t>(50, 0), "all empty")) return false;
    if (!check_tiles({T + 1}, "one large")) return false;
    if (!check_tiles({0, 0, T + 1, 0, 0, 5, 0}, "large then small")) return false;
    if (!check_tiles({5, T + 1}, "small then large")) return false;
    return true;
}

// off(q) computed, nothing stored: nq = 2^32 - 1 and offsets above 2^32
struct SynthOff {
    uint64_t per, period;   // every period-th query has `per` hits, the others none
    uint64_t operator()(uint64_t q) const { return ((q + period - 1) / period) * per; }
};

static bool check_synthetic() {
    const uint64_t nq = 0xFFFFFFFFull;
    const uint64_t pers[] = {1, 3, 16, T - 1, T, T + 1, 5 * T};
    const uint64_t periods[] = {1, 2, 1000};
    std::mt19937_64 rng(99);
    for (uint64_t per : pers)
        for (uint64_t period : periods) {
            const SynthOff off{per, period};
            const uint64_t total = off(nq), tiles = (total + T - 1) / T;
            if (period == 1 && per >= 3 && total <= (1ull << 32)) FAIL("synthetic total too small");
            for (int k = 0; k < 200; ++k) {
                const uint64_t t = k < 4 ? (uint64_t)k : k < 8 ? tiles - (k - 3) : rng() % tiles;
                // the non-empty queries are g * period (g = 0, 1, ...), starting at g * per:
                // the tile's first is the smallest g with g * per >= t * T
                const uint64_t g0 = (t * T + per - 1) / per, g1 = ((t + 1) * T + per - 1) / per;
                const uint64_t last_g = (nq - 1) / period;   // the last non-empty query's g
                // first query index with off >= t * T: off(q) = ceil(q / period) * per
                uint64_t want_q0 = g0 == 0 ? 0 : (g0 - 1) * period + 1;
                if (want_q0 > nq) want_q0 = nq;
                const sa::LocateTile r = sa::locate_tile(off, nq, t);
                if (r.q0 != want_q0) FAIL("synthetic per %llu period %llu tile %llu: q0 %llu want %llu", (ull)per,
                                          (ull)period, (ull)t, (ull)r.q0, (ull)want_q0);
                const uint64_t ng = g0 > last_g ? 0 : std::min(g1, last_g + 1) - g0;   // queries that start in the tile
                const uint64_t want_hits = per > T ? 0 : ng * per;
                if (r.e - r.s != want_hits) FAIL("synthetic per %llu period %llu tile %llu: %llu hits want %llu",
                                                 (ull)per, (ull)period, (ull)t, (ull)(r.e - r.s), (ull)want_hits);
                if (want_hits && r.s != g0 * per) FAIL("synthetic start");
                if (r.e - r.s >= 2 * T) FAIL("synthetic tile too full");
                ++g_cases;
            }
        }
    return true;
}

static bool check_keys() {
    const uint64_t n = 0xFFFFFFFFull;
    if (sa::locate_bits(0) != 0 || sa::locate_bits(1) != 0 || sa::locate_bits(2) != 1 || sa::locate_bits(3) != 2 ||
        sa::locate_bits(256) != 8 || sa::locate_bits(257) != 9 || sa::locate_bits(n) != 32 ||
        sa::locate_bits(1ull << 32) != 32 || sa::locate_bits((1ull << 32) + 1) != 33)
        FAIL("locate_bits");
    const uint64_t nls[] = {1, 2, 256, 257};
    const uint32_t want_bits[] = {32, 33, 40, 41};
    std::mt19937_64 rng(7);
    for (int k = 0; k < 4; ++k) {
        const uint64_t nl = nls[k];
        if (sa::locate_key_bits(n, nl) != want_bits[k]) FAIL("key bits at n_large %llu", (ull)nl);
        const uint32_t pb = sa::locate_bits(n);
        uint64_t pj = 0, pk = 0;
        uint32_t pp = 0;
        for (int i = 0; i < 2000; ++i) {
            const uint64_t j = i < 2 ? (i ? nl - 1 : 0) : rng() % nl;
            const uint32_t p = i < 4 ? (i & 1 ? 0xFFFFFFFEu : 0u) : (uint32_t)rng() % 0xFFFFFFFFu;
            const uint64_t key = sa::locate_key(j, p, pb);
            if (sa::locate_key_query(key, pb) != j || sa::locate_key_pos(key, pb) != p) FAIL("key round trip");
            if (want_bits[k] < 64 && (key >> want_bits[k])) FAIL("key wider than its bit count");
            if (i && ((key < pk) != (j < pj || (j == pj && p < pp)))) FAIL("key order");
            pj = j;
            pp = p;
            pk = key;
            ++g_cases;
        }
    }
    // a smaller n: positions in bits(n) bits
    if (sa::locate_key_bits(1 << 20, 300) != 20 + 9) FAIL("key bits at 2^20");
    if (sa::locate_key_pos(sa::locate_key(299, (1 << 20) - 1, 20), 20) != (1 << 20) - 1) FAIL("key at 2^20");
    return true;
}

static bool check_split() {
    for (uint32_t first = 0; first < 4; ++first)
        for (uint64_t total = 0; total < 10; ++total) {
            const sa::LocateSplit s = sa::locate_split(first, total);
            // whole 16-byte groups inside entries [first, first + total) of the line
            uint64_t groups = 0;
            for (uint64_t g = 0; g < 8; ++g) groups += 4 * g >= first && 4 * g + 4 <= first + total;
            if (s.head + s.body + s.tail != total || s.body != 4 * groups || s.head > 3 || s.tail > 3)
                FAIL("split first %u total %llu: %u %llu %u", first, (ull)total, s.head, (ull)s.body, s.tail);
            if (s.body && ((first + s.head) & 3u)) FAIL("split body not aligned");
            if (!s.body && s.head + s.tail != total) FAIL("split without body");
            ++g_cases;
        }
    const sa::LocateSplit s = sa::locate_split(3, (1ull << 33) + 2);
    if (s.head != 1 || s.body != (1ull << 33) || s.tail != 1) FAIL("split above 2^32");
    return true;
}

int main() {
    if (!check_counts() || !check_random_tiles() || !check_synthetic() || !check_keys() || !check_split()) return 1;
    std::printf("ok %ld\n", g_cases);
    return 0;
}
