// Host check of the host-compilable core of the LF-mapping and the inverse BWT
// (hpc_suffix_array_amd/csrc/sa_ibwt.h).  The kernels' steps run here one after
// the other on the host, over the same functions: LF from per-tile counts, a
// scan per byte across tiles and in-tile ranks with the primary row apart
// (tiles of 8 and of 1000 ranks); first[] and the byte search; the splitter
// words, word counts and tile sums (256 words per tile as on the device, and
// 2); walk 1 from every splitter; pointer jumping between two buffers; the
// verdict; walk 2 with its byte packing at the four alignments of the output.
// With one rank in 64 a splitter (the product) and one in 4 (so that lists of
// many splitters and several rounds run at these sizes).
// Against brute force: LF by a stable sort of the reordered rows, the verdict
// and the steps by following the chain, text and SA by a naive suffix sort.
//   * every (bwt, p) over {a,b}^n, n <= 10: accepted iff it is the image of a
//     text, which then comes back with its SA;
//   * texts of 0 .. 300 bytes over alphabets of 1, 2, 4 and 256 symbols, and
//     random bytes with a random primary index;
//   * the arithmetic at n = 2^32 - 1 on accessors with no memory behind them.
// Every array is an exact-size heap allocation, so a build with
// -fsanitize=address sees any access past an end.  Prints
// "ok <checks> checks on <texts> texts, <valid> valid of <pairs> pairs" or the
// first mismatch.  Built by tests/test_ibwt_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "sa_ibwt.h"

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

typedef std::vector<uint8_t> Bytes;

static std::vector<uint32_t> naive_sa(const Bytes& t) {
    std::vector<uint32_t> sa(t.size());
    std::iota(sa.begin(), sa.end(), 0u);
    const std::string_view v((const char*)t.data(), t.size());
    std::sort(sa.begin(), sa.end(), [&](uint32_t a, uint32_t b) {
        const std::string_view x = v.substr(a), y = v.substr(b);
        const size_t m = std::min(x.size(), y.size());
        const int c = std::memcmp(x.data(), y.data(), m);
        return c ? c < 0 : x.size() < y.size();
    });
    return sa;
}

static void naive_bwt(const Bytes& t, const std::vector<uint32_t>& sa, Bytes& bwt, uint32_t& p) {
    const size_t n = t.size();
    bwt.resize(n);
    for (size_t r = 0; r < n; ++r) {
        if (sa[r] == 0) p = (uint32_t)r;
        bwt[r] = t[sa[r] ? sa[r] - 1 : n - 1];
    }
}

// the definition: rows p, 0, 1, .. without p, sorted stably by byte
static std::vector<uint32_t> brute_lf(const Bytes& bwt, uint32_t p) {
    const uint32_t n = (uint32_t)bwt.size();
    std::vector<uint32_t> rows;
    rows.push_back(p);
    for (uint32_t r = 0; r < n; ++r)
        if (r != p) rows.push_back(r);
    std::stable_sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) { return bwt[a] < bwt[b]; });
    std::vector<uint32_t> lf(n);
    for (uint32_t i = 0; i < n; ++i) lf[rows[i]] = i;
    return lf;
}

// LF as the three kernels compute it, with tiles of `tile` ranks
static bool kernel_lf(const Bytes& bwt, uint32_t p, uint32_t tile, Heap<uint32_t>& lf, Heap<uint32_t>& first) {
    const uint32_t n = (uint32_t)bwt.size();
    const uint32_t tiles = (n + tile - 1) / tile;
    Heap<uint32_t> cnt((uint64_t)256 * tiles), totals(256), e(256);
    for (uint64_t i = 0; i < cnt.n; ++i) cnt[i] = 0;
    for (uint32_t r = 0; r < n; ++r)
        if (r != p) ++cnt[(uint64_t)bwt[r] * tiles + r / tile];
    for (uint32_t c = 0; c < 256; ++c) {   // k_lf_scan
        uint32_t run = 0;
        for (uint32_t t = 0; t < tiles; ++t) {
            const uint32_t y = cnt[(uint64_t)c * tiles + t];
            cnt[(uint64_t)c * tiles + t] = run;
            run += y;
        }
        totals[c] = run;
    }
    uint32_t run = 0;
    for (uint32_t c = 0; c < 256; ++c) {
        e[c] = run;
        run += totals[c];
    }
    if (run != n - 1) FAIL("totals sum to %u, n - 1 = %u", run, n - 1);
    const uint32_t last = bwt[p];
    for (uint32_t c = 0; c < 256; ++c) first[c] = sa::lf_first(e[c], c, last);
    first[256] = n;
    lf[p] = e[last];
    for (uint32_t t = 0; t < tiles; ++t) {   // k_lf_rank
        Heap<uint32_t> s_c(256);
        for (uint32_t c = 0; c < 256; ++c) s_c[c] = sa::lf_base(e[c], c, last) + cnt[(uint64_t)c * tiles + t];
        for (uint32_t r = t * tile; r < std::min(n, (t + 1) * tile); ++r)
            if (r != p) lf[r] = s_c[bwt[r]]++;
    }
    return true;
}

template <uint32_t WPT>
struct Dir {
    Heap<uint64_t> words;
    Heap<uint32_t> wcnt;
    Heap<uint64_t> tinc;
    Dir(uint64_t nw, uint64_t nt) : words(nw), wcnt(nw), tinc(nt) {}
    uint64_t word(uint32_t w) const { return words[w]; }
    uint64_t count(uint32_t w) const { return wcnt[w]; }
    uint64_t tile(uint32_t t) const { return t ? tinc[t - 1] : 0; }
};

struct Out {
    Heap<uint8_t>& text;
    Heap<uint32_t>& sa_out;
    Heap<uint8_t>& hits;   // how often each byte was written
    uint32_t addr;
    bool bad = false;
    long words = 0;
    void byte(uint32_t q, uint32_t b) {
        text[q] = (uint8_t)b;
        ++hits[q];
    }
    void word(uint32_t q, uint32_t x) {
        if ((addr + q) & 3u) bad = true;
        for (uint32_t k = 0; k < 4; ++k) byte(q + k, (x >> (8 * k)) & 255u);
        ++words;
    }
    void sa(uint32_t r, uint32_t q) { sa_out[r] = q; }
};

struct Result {
    bool valid = false;
    uint64_t splitters = 0, longest = 0, steps = 0;
    Bytes text;
    std::vector<uint32_t> sa;
};

// the whole inversion, step by step as sa_ibwt_device enqueues it
template <uint32_t WPT>
static bool invert(const Bytes& bwt, uint32_t p, uint32_t bits, uint32_t lf_tile, uint32_t addr, Result& res) {
    const uint32_t n = (uint32_t)bwt.size();
    Heap<uint32_t> lf(n), first(257);
    if (!kernel_lf(bwt, p, lf_tile, lf, first)) return false;
    const std::vector<uint32_t> want_lf = brute_lf(bwt, p);
    for (uint32_t r = 0; r < n; ++r) {
        ++g_checks;
        if (lf[r] != want_lf[r]) FAIL("LF[%u] = %u, stable sort says %u (n %u p %u)", r, lf[r], want_lf[r], n, p);
        if (sa::ibwt_byte_of(first.p.get(), lf[r]) != bwt[r])
            FAIL("byte of rank %u: %u, bwt[%u] = %u", lf[r], sa::ibwt_byte_of(first.p.get(), lf[r]), r, bwt[r]);
    }
    const auto lf_at = [&](uint32_t r) { return lf[r]; };
    const uint32_t r0 = lf[p];
    // the directory
    const uint64_t nw = ((uint64_t)n + 63) / 64, nt = (nw + WPT - 1) / WPT;
    Dir<WPT> d(nt * WPT, nt);
    uint64_t total = 0;
    for (uint64_t t = 0; t < nt; ++t) {
        uint32_t in_tile = 0;
        for (uint32_t k = 0; k < WPT; ++k) {
            const uint64_t w = t * WPT + k;
            d.words[w] = sa::ibwt_split_word(w, n, r0, bits);
            d.wcnt[w] = in_tile;
            in_tile += (uint32_t)__builtin_popcountll(d.words[w]);
        }
        total += in_tile;
        d.tinc[t] = total;
    }
    uint32_t seen = 0;
    for (uint32_t r = 0; r < n; ++r) {
        ++g_checks;
        const bool is = sa::ibwt_is_splitter(r, r0, bits);
        if (is != (bool)((d.words[r / 64] >> (r % 64)) & 1)) FAIL("splitter bit of rank %u", r);
        if (sa::ibwt_dir_index<WPT>(d, r) != seen) FAIL("index of rank %u: %u, %u below it", r, sa::ibwt_dir_index<WPT>(d, r), seen);
        seen += is;
    }
    const uint64_t m = total;
    if (m != seen || m == 0) FAIL("%llu splitters, %u bits set", (ull)m, seen);
    // walk 1: the j-th splitter by selection, as a lane finds it
    Heap<uint64_t> na(m), nb(m);
    uint64_t j = 0, longest = 0, sum = 0;
    for (uint64_t w = 0; w < nw; ++w)
        for (uint32_t k = 0; k < (uint32_t)__builtin_popcountll(d.words[w]); ++k, ++j) {
            const uint32_t s = sa::ibwt_select(d.words[w], k, (uint32_t)w);
            if (!sa::ibwt_is_splitter(s, r0, bits) || sa::ibwt_dir_index<WPT>(d, s) != j) FAIL("select %u of word %llu", k, (ull)w);
            uint32_t end;
            const uint32_t len = sa::ibwt_walk1(lf_at, s, r0, bits, n, end);
            na[j] = sa::ibwt_node(end == r0 ? sa::kIbwtNil : sa::ibwt_dir_index<WPT>(d, end), len);
            longest = std::max<uint64_t>(longest, len);
            sum += len;
        }
    if (sum > n) FAIL("sublists hold %llu ranks of %u", (ull)sum, n);   // (a cycle without a splitter is in none)
    // pointer jumping, two buffers; one round more than needed changes nothing
    const int rounds = sa::ibwt_rounds(m);
    if ((1ull << rounds) < m || (rounds && (1ull << (rounds - 1)) >= m)) FAIL("rounds(%llu) = %d", (ull)m, rounds);
    Heap<uint64_t>*in = &na, *out = &nb;
    for (int k = 0; k < rounds + 1; ++k) {
        for (uint64_t i = 0; i < m; ++i) (*out)[i] = sa::ibwt_jump(in->p.get(), (*in)[i]);
        if (k == rounds)
            for (uint64_t i = 0; i < m; ++i)
                if (sa::ibwt_succ((*in)[i]) == sa::kIbwtNil && (*out)[i] != (*in)[i]) FAIL("a finished node moved");
        std::swap(in, out);
    }
    const uint64_t L = sa::ibwt_dist((*in)[sa::ibwt_dir_index<WPT>(d, r0)]);
    // brute force: follow the chain from r0 until p
    uint64_t steps = 0;
    for (uint32_t r = r0; r != p; r = lf[r]) ++steps;
    ++g_checks;
    if (L != steps + 1) FAIL("cycle of r0: %llu, chain says %llu (n %u p %u bits %u)", (ull)L, (ull)steps + 1, n, p, bits);
    res.valid = L == n;
    res.splitters = m;
    res.longest = longest;
    res.steps = L - 1;
    if (!res.valid) return true;
    if (sum != n) FAIL("one cycle of %u ranks, sublists of %llu", n, (ull)sum);
    // walk 2
    Heap<uint8_t> text(n), hits(n);
    Heap<uint32_t> sa_out(n);
    for (uint32_t i = 0; i < n; ++i) hits[i] = 0, text[i] = 0, sa_out[i] = ~0u;
    Out o{text, sa_out, hits, addr};
    j = 0;
    for (uint64_t w = 0; w < nw; ++w)
        for (uint32_t k = 0; k < (uint32_t)__builtin_popcountll(d.words[w]); ++k, ++j) {
            const uint32_t dist = sa::ibwt_dist((*in)[j]);
            if (dist == 0 || dist > n) FAIL("splitter %llu at distance %u", (ull)j, dist);
            sa::ibwt_walk2(lf_at, first.p.get(), sa::ibwt_select(d.words[w], k, (uint32_t)w), dist - 1, r0, bits, n, addr, o);
        }
    if (o.bad) FAIL("a dword store at an address that is not a multiple of 4");
    for (uint32_t i = 0; i < n; ++i)
        if (hits[i] != 1) FAIL("text[%u] written %u times (n %u addr %u)", i, hits[i], n, addr);
    if (n >= 64 && bits == sa::kIbwtSplitBits && o.words * 4 < (long)n / 2) FAIL("only %ld dword stores for %u bytes", o.words, n);
    // the definition: follow the chain
    Bytes want(n);
    std::vector<uint32_t> want_sa(n);
    uint32_t r = r0;
    want[n - 1] = bwt[p];
    want_sa[r] = n - 1;
    for (uint32_t k = 1; k < n; ++k) {
        want[n - 1 - k] = bwt[r];
        r = lf[r];
        want_sa[r] = n - 1 - k;
    }
    res.text.assign(text.p.get(), text.p.get() + n);
    res.sa.assign(sa_out.p.get(), sa_out.p.get() + n);
    g_checks += n;
    if (res.text != want) FAIL("text differs from the chain's (n %u p %u bits %u addr %u)", n, p, bits, addr);
    if (res.sa != want_sa) FAIL("SA differs from the chain's (n %u p %u bits %u)", n, p, bits);
    return true;
}

static long g_texts = 0, g_pairs = 0, g_valid = 0;

// a text: its BWT comes back as the text and its SA, under every setting
static bool round_trip(const Bytes& t) {
    ++g_texts;
    if (t.empty()) return true;
    const std::vector<uint32_t> sa = naive_sa(t);
    Bytes bwt;
    uint32_t p = 0;
    naive_bwt(t, sa, bwt, p);
    for (uint32_t bits : {sa::kIbwtSplitBits, 2u})
        for (uint32_t addr = 0; addr < 4; ++addr) {
            Result a, b;
            if (!invert<sa::kIbwtTileWords>(bwt, p, bits, 1000, addr, a) || !invert<2>(bwt, p, bits, 8, addr, b)) return false;
            for (const Result* r : {&a, &b}) {
                if (!r->valid) FAIL("the BWT of a text of %zu bytes is rejected", t.size());
                if (r->text != t || r->sa != sa) FAIL("round trip of %zu bytes (bits %u addr %u)", t.size(), bits, addr);
                if (r->steps != t.size() - 1) FAIL("steps %llu", (ull)r->steps);
            }
            if (a.splitters != b.splitters || a.longest != b.longest) FAIL("the tiling changes the splitters");
        }
    return true;
}

static bool exhaustive() {
    for (uint32_t n = 1; n <= 10; ++n) {
        std::set<std::pair<Bytes, uint32_t>> images;
        for (uint32_t x = 0; x < (1u << n); ++x) {
            Bytes t(n);
            for (uint32_t i = 0; i < n; ++i) t[i] = (x >> i) & 1 ? 'b' : 'a';
            Bytes bwt;
            uint32_t p = 0;
            naive_bwt(t, naive_sa(t), bwt, p);
            if (!images.insert({bwt, p}).second) FAIL("two texts share a BWT");
        }
        for (uint32_t x = 0; x < (1u << n); ++x) {
            Bytes bwt(n);
            for (uint32_t i = 0; i < n; ++i) bwt[i] = (x >> i) & 1 ? 'b' : 'a';
            for (uint32_t p = 0; p < n; ++p) {
                ++g_pairs;
                Result a, b;
                if (!invert<sa::kIbwtTileWords>(bwt, p, sa::kIbwtSplitBits, 1000, p & 3, a) || !invert<2>(bwt, p, 2, 8, x & 3, b)) return false;
                const bool image = images.count({bwt, p}) != 0;
                if (a.valid != image || b.valid != image) FAIL("n %u bwt %#x p %u: accepted %d %d, an image %d", n, x, p, a.valid, b.valid, image);
                if (a.steps != b.steps) FAIL("steps differ with the splitters");
                if (!image) {
                    if (a.steps >= n - 1) FAIL("an invalid pair with %llu steps", (ull)a.steps);
                    continue;
                }
                ++g_valid;
                Bytes back;
                uint32_t q = 0;
                naive_bwt(a.text, naive_sa(a.text), back, q);
                if (back != bwt || q != p || a.text != b.text || a.sa != naive_sa(a.text) || b.sa != a.sa) FAIL("n %u bwt %#x p %u decodes to another text", n, x, p);
            }
        }
    }
    return true;
}

// n = 2^32 - 1: no memory behind the accessors
static bool arithmetic() {
    const uint64_t n = 0xFFFFFFFFull;
    g_checks += 12;
    if (sa::lf_first((uint32_t)(n - 1), 255, 3) != n || sa::lf_base((uint32_t)(n - 1), 255, 255) != n) FAIL("first / base at the top");
    if (sa::lf_base(0, 0, 0) != 1 || sa::lf_first(0, 0, 0) != 0 || sa::lf_base(7, 2, 3) != 7 || sa::lf_first(7, 4, 3) != 8) FAIL("first / base");
    const uint64_t cap = sa::ibwt_node_cap(n);
    if (cap < n / 64 + 1 || cap > n / 32 || sa::ibwt_rounds(cap) != 27 || sa::ibwt_rounds(1) != 0 || sa::ibwt_rounds(2) != 1 || sa::ibwt_rounds(1025) != 11)
        FAIL("cap %llu, rounds %d", (ull)cap, sa::ibwt_rounds(cap));
    const uint64_t wl = (n - 1) / 64;   // the last word: 63 ranks
    const uint64_t word = sa::ibwt_split_word(wl, n, (uint32_t)(n - 1), sa::kIbwtSplitBits);
    if (!((word >> 62) & 1) || (word >> 63)) FAIL("the last word: %#llx", (ull)word);
    for (uint32_t k = 0; k < 63; ++k)
        if ((bool)((word >> k) & 1) != sa::ibwt_is_splitter((uint32_t)(wl * 64 + k), (uint32_t)(n - 1), sa::kIbwtSplitBits)) FAIL("bit %u of the last word", k);
    // the hash keeps one rank in 2^bits, evenly: every stretch of 2^20 ranks
    for (uint32_t base : {0u, 0x7FF00000u, 0xFFE00000u})
        for (uint32_t bits : {2u, 6u}) {
            uint32_t c = 0;
            for (uint32_t r = 0; r < (1u << 20); ++r) c += sa::ibwt_hashed(base + r, bits);
            const uint32_t want = (1u << 20) >> bits;
            if (c + 64 < want || c > want + 64) FAIL("%u of 2^20 ranks from %#x hash to a splitter (bits %u)", c, base, bits);
        }
    struct {
        uint64_t word(uint32_t) const { return ~0ull; }
        uint64_t count(uint32_t w) const { return (w % 256) * 64ull; }
        uint64_t tile(uint32_t t) const { return t * 16384ull; }
    } full;
    if (sa::ibwt_dir_index<256>(full, (uint32_t)(n - 1)) != n - 1 || sa::ibwt_dir_index<256>(full, 0) != 0) FAIL("index at the top");
    if (sa::ibwt_select(1ull << 62, 0, (uint32_t)wl) != n - 1 || sa::ibwt_select(~0ull, 63, 5) != 5 * 64 + 63) FAIL("select");
    Heap<uint32_t> first(257);
    for (uint32_t c = 0; c < 257; ++c) first[c] = c < 200 ? 0u : c < 256 ? (uint32_t)(n - 1) : (uint32_t)n;
    if (sa::ibwt_byte_of(first.p.get(), (uint32_t)(n - 1)) != 255 || sa::ibwt_byte_of(first.p.get(), (uint32_t)(n - 2)) != 199 || sa::ibwt_byte_of(first.p.get(), 0) != 199)
        FAIL("byte search");
    // LF[r] = r + 1 mod n: the chain runs up the ranks
    const auto up = [&](uint32_t r) { return (uint64_t)r + 1 == n ? 0u : r + 1; };
    uint32_t end = 0;
    const uint32_t s = (uint32_t)(n - 5);
    uint32_t len = sa::ibwt_walk1(up, s, 2, 6, n, end);
    uint32_t want = 0, r = s;
    do {
        r = up(r);
        ++want;
    } while (!sa::ibwt_is_splitter(r, 2, 6));
    if (len != want || end != r) FAIL("walk 1 across the top: %u steps to %u, want %u to %u", len, end, want, r);
    if (sa::ibwt_dist(sa::ibwt_node(sa::kIbwtNil, (uint32_t)n)) != n || sa::ibwt_succ(sa::ibwt_node(sa::kIbwtNil - 1, 7)) != sa::kIbwtNil - 1) FAIL("node");
    struct Count {
        uint64_t lo = ~0ull, hi = 0, bytes = 0;
        void byte(uint32_t q, uint32_t) { lo = std::min<uint64_t>(lo, q), hi = std::max<uint64_t>(hi, q), ++bytes; }
        void word(uint32_t q, uint32_t) { lo = std::min<uint64_t>(lo, q), hi = std::max<uint64_t>(hi, (uint64_t)q + 3), bytes += 4; }
        void sa(uint32_t, uint32_t) {}
    } cnt;
    sa::ibwt_walk2(up, first.p.get(), s, (uint32_t)(n - 1), 2, 6, n, 1, cnt);
    if (cnt.hi != n - 1 || cnt.bytes != len || cnt.lo != n - len) FAIL("walk 2 at the top: [%llu, %llu], %llu bytes, %u steps", (ull)cnt.lo, (ull)cnt.hi, (ull)cnt.bytes, len);
    return true;
}

int main() {
    if (!arithmetic() || !exhaustive()) return 1;
    std::mt19937_64 rng(20261020);
    for (uint32_t sigma : {1u, 2u, 4u, 256u})
        for (uint32_t n = 0; n <= 300; n += n < 70 ? 1 : 23) {
            Bytes t(n);
            for (auto& b : t) b = sigma == 256 ? (uint8_t)rng() : (uint8_t)("acgt"[rng() % sigma]);
            if (!round_trip(t)) return 1;
        }
    for (const char* s : {"banana", "mississippi", "abracadabra", "aaaaaaaab", "baaaaaaaa", "abababababababab"}) {
        const Bytes t((const uint8_t*)s, (const uint8_t*)s + std::strlen(s));
        if (!round_trip(t)) return 1;
    }
    {   // Thue-Morse and (1..64)^k, 2048 bytes
        Bytes tm(2048), per(2048);
        for (uint32_t i = 0; i < 2048; ++i) tm[i] = 'a' + (__builtin_popcount(i) & 1), per[i] = 1 + i % 64;
        if (!round_trip(tm) || !round_trip(per)) return 1;
    }
    // any bytes, any primary: a permutation, a verdict, no access past an end
    for (uint32_t n : {1u, 2u, 3u, 17u, 64u, 65u, 129u, 300u, 1000u, 4097u})
        for (uint32_t sigma : {1u, 2u, 4u, 256u})
            for (int rep = 0; rep < 3; ++rep) {
                Bytes b(n);
                for (auto& x : b) x = (uint8_t)(rng() % sigma);
                ++g_pairs;
                Result a, c;
                const uint32_t p = (uint32_t)(rng() % n);
                if (!invert<sa::kIbwtTileWords>(b, p, sa::kIbwtSplitBits, 1000, rep, a) || !invert<2>(b, p, 2, 8, rep, c)) return 1;
                if (a.valid != c.valid || a.steps != c.steps) {
                    std::printf("FAIL random pair n %u: verdicts differ\n", n);
                    return 1;
                }
                g_valid += a.valid;
            }
    std::printf("ok %ld checks on %ld texts, %ld valid of %ld pairs\n", g_checks, g_texts, g_valid, g_pairs);
    return 0;
}
