// Host check of the host-compilable core of the longest previous factor array
// and the LZ77 parse (hpc_suffix_array_amd/csrc/sa_lz.h).
//   LPF: the nearest-smaller walks with LCP minima over a hierarchy built here
//   on the host, with fan-out 64 and with fan-out 4 (three and more levels at
//   these sizes), whole and as the kernel composes them (a window of F * F
//   ranks first, then the whole hierarchy from the window's edge), against
//   the O(n^2) definition of LPF and the canonical SRC of include/sa_hip.h.
//   Parse: exits by pointer jumping per tile (B = 4, 8, 16), the candidates,
//   their successors, the reach rounds, the entries, the marks by doubling and
//   the emitted phrases, against the serial walk, on LPF arrays of texts and
//   on arbitrary ones.
//   The 64-bit clamp of next() and the walks at n = 2^32 - 1 run on accessors
//   with no memory behind them.
// Every array is an exact-size heap allocation of 0 .. 300 entries, so a build
// with -fsanitize=address sees any access past an end.  Prints "ok <checks>"
// or the first mismatch.  Built by tests/test_lz_core.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "sa_lz.h"

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

// the hierarchy over ranks [lo, lo + len) of (sa, lcp), levels up to one node
template <uint32_t F>
struct Hier {
    std::vector<Heap<sa::LpfNode>> lv;
    int n_levels = 0;
    mutable long reads = 0;
    Hier(const Heap<uint32_t>& s, const Heap<uint32_t>& l, uint64_t lo, uint64_t len, int force_levels = 0) {
        uint64_t cnt[sa::kLpfMaxLevels];
        n_levels = sa::lpf_level_counts<F>(len, cnt);
        if (force_levels)   // the kernel's window: always three levels
            for (; n_levels < force_levels; ++n_levels) cnt[n_levels] = 1;
        for (int k = 0; k < n_levels; ++k) lv.emplace_back(cnt[k]);
        for (uint64_t i = 0; i < len; ++i) lv[0][i] = sa::LpfNode{s[lo + i], l[lo + i]};
        for (int k = 1; k < n_levels; ++k)
            for (uint64_t p = 0; p < lv[k].n; ++p) {
                sa::LpfNode m{~0u, ~0u};
                for (uint64_t c = p * F; c < std::min<uint64_t>(p * F + F, lv[k - 1].n); ++c) {
                    m.sa = std::min(m.sa, lv[k - 1][c].sa);
                    m.lcp = std::min(m.lcp, lv[k - 1][c].lcp);
                }
                lv[k][p] = m;
            }
    }
    int levels() const { return n_levels; }
    uint64_t count(int k) const { return lv[k].n; }
    sa::LpfNode operator()(int k, uint64_t i) const {
        ++reads;
        if (k < 0 || k >= n_levels || i >= lv[k].n) {
            std::printf("FAIL node (%d, %llu) read\n", k, (ull)i);
            std::abort();
        }
        return lv[k][i];
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

static uint64_t common(const std::vector<uint8_t>& t, uint64_t a, uint64_t b) {
    uint64_t k = 0;
    while (a + k < t.size() && b + k < t.size() && t[a + k] == t[b + k]) ++k;
    return k;
}

// the kernel's composition: the window that holds r first, then the whole
template <uint32_t F>
static void resolve(const Hier<F>& g, const Hier<F>& win, uint64_t base, uint64_t r, uint32_t v, uint32_t lcp_r,
                    uint32_t& lpf, uint32_t& src) {
    uint32_t la = lcp_r, va = 0, lb = ~0u, vb = 0;
    bool fa = sa::lpf_walk_left<F, 1>(win, r - base, v, la, va);
    if (!fa) fa = sa::lpf_walk_left<F, sa::kLpfChunk>(g, base, v, la, va);
    bool fb = sa::lpf_walk_right<F, 1>(win, r - base, v, lb, vb);
    if (!fb) fb = sa::lpf_walk_right<F, sa::kLpfChunk>(g, base + win.count(0) - 1, v, lb, vb);
    sa::lpf_combine(fa, la, va, fb, lb, vb, lpf, src);
}

template <uint32_t F>
static bool check_lpf(const std::vector<uint8_t>& t, const Heap<uint32_t>& s, const Heap<uint32_t>& l,
                      const std::vector<uint32_t>& want_lpf, const std::vector<uint32_t>& want_src) {
    const uint64_t n = t.size();
    if (n == 0) return true;
    const Hier<F> g(s, l, 0, n);
    const uint64_t W = (uint64_t)F * F;
    for (uint64_t base = 0; base < n; base += W) {
        const uint64_t len = std::min<uint64_t>(W, n - base);
        const Hier<F> win(s, l, base, len, 3);
        for (uint64_t r = base; r < base + len; ++r) {
            const uint32_t v = s[r];
            // whole, one node a step and kLpfChunk nodes a step
            uint32_t la = l[r], va = 0, lb = ~0u, vb = 0, lpf, src;
            g.reads = 0;
            bool fa = sa::lpf_walk_left<F, 1>(g, r, v, la, va);
            bool fb = sa::lpf_walk_right<F, 1>(g, r, v, lb, vb);
            if (g.reads > 2L * 2 * F * g.levels())
                FAIL("F=%u n=%llu rank %llu: %ld reads for %d levels", F, (ull)n, (ull)r, g.reads, g.levels());
            sa::lpf_combine(fa, la, va, fb, lb, vb, lpf, src);
            if (lpf != want_lpf[v] || src != want_src[v])
                FAIL("F=%u n=%llu i=%u: walk gives (%u, %u), the definition (%u, %u)", F, (ull)n, v, lpf, src,
                     want_lpf[v], want_src[v]);
            la = l[r], lb = ~0u;
            fa = sa::lpf_walk_left<F, sa::kLpfChunk>(g, r, v, la, va);
            fb = sa::lpf_walk_right<F, sa::kLpfChunk>(g, r, v, lb, vb);
            sa::lpf_combine(fa, la, va, fb, lb, vb, lpf, src);
            if (lpf != want_lpf[v] || src != want_src[v])
                FAIL("F=%u n=%llu i=%u: chunked walk gives (%u, %u), the definition (%u, %u)", F, (ull)n, v, lpf, src,
                     want_lpf[v], want_src[v]);
            // window, then the whole from its edge
            resolve<F>(g, win, base, r, v, l[r], lpf, src);
            if (lpf != want_lpf[v] || src != want_src[v])
                FAIL("F=%u n=%llu i=%u: window walk gives (%u, %u), the definition (%u, %u)", F, (ull)n, v, lpf,
                     src, want_lpf[v], want_src[v]);
            g_checks += 3;
        }
    }
    return true;
}

static std::vector<std::vector<uint32_t>> serial_parse(const Heap<uint32_t>& lpf, const Heap<uint32_t>& src, uint64_t n) {
    std::vector<std::vector<uint32_t>> out;
    for (uint64_t i = 0; i < n;) {
        const uint64_t nx = sa::lz_next(i, lpf[i], n);
        out.push_back({(uint32_t)i, (uint32_t)(nx - i), lpf[i] ? src[i] : sa::kLpfNone});
        i = nx;
    }
    return out;
}

// the phases of lz77_device with tiles of B positions
static bool check_parse(const Heap<uint32_t>& lpf, const Heap<uint32_t>& src, uint64_t n, uint32_t B, const char* what) {
    const auto want = serial_parse(lpf, src, n);
    if (n == 0) return want.empty();
    int rounds = 0;
    while ((1u << rounds) < B) ++rounds;
    const uint64_t tiles = (n + B - 1) / B;
    Heap<uint32_t> exit(n);
    Heap<uint8_t> mask(n);
    for (uint64_t i = 0; i < n; ++i) mask[i] = 0;
    for (uint64_t t = 0; t < tiles; ++t) {
        const uint64_t base = t * B, end = std::min<uint64_t>(base + B, n);
        Heap<uint32_t> e(B);
        for (uint32_t i = 0; i < B; ++i) e[i] = base + i < n ? (uint32_t)sa::lz_next(base + i, lpf[base + i], n) : (uint32_t)n;
        for (int k = 0; k < rounds; ++k)
            for (uint32_t i = 0; i < B; ++i)   // in place, in one of the orders the lanes may take
                e[i] = sa::lz_jump(e[i], base, end, [&](uint32_t x) { return e[x]; });
        for (uint32_t i = 0; base + i < end; ++i) {
            if (e[i] < end) FAIL("%s n=%llu B=%u: exit of %llu is %u, inside its tile", what, (ull)n, B, (ull)(base + i), e[i]);
            exit[base + i] = e[i];
            if (e[i] < n && (i == 0 || e[i - 1] != e[i])) mask[e[i]] = 1;
        }
    }
    mask[0] = 1;
    std::vector<int64_t> cand_v;
    for (uint64_t i = 0; i < n; ++i)
        if (mask[i]) cand_v.push_back((int64_t)i);
    const uint64_t c = cand_v.size();
    Heap<int64_t> cand(c);
    for (uint64_t k = 0; k < c; ++k) cand[k] = cand_v[k];
    const auto cand_at = [&](uint64_t k) { return (uint64_t)cand[k]; };
    Heap<uint32_t> j0(c + 1), j1(c + 1), flag(c + 1);
    for (uint64_t k = 0; k <= c; ++k) {
        j0[k] = (uint32_t)(k < c ? sa::lz_cand_succ(cand_at, c, exit[cand[k]], n) : c);
        flag[k] = k == 0;
        if (k < c && j0[k] < c && (uint64_t)cand[j0[k]] != exit[cand[k]])
            FAIL("%s n=%llu B=%u: successor of candidate %llu", what, (ull)n, B, (ull)k);
    }
    Heap<uint32_t>* cur = &j0;
    Heap<uint32_t>* nxt = &j1;
    for (int t = 0; t < sa::lz_reach_rounds(c); ++t) {
        for (uint64_t k = 0; k <= c; ++k) {
            const uint64_t j = std::min<uint64_t>((*cur)[k], c);
            if (j < c && flag[k]) flag[j] = 1;   // in place: seen early by the later k
            (*nxt)[k] = (*cur)[j];
        }
        std::swap(cur, nxt);
    }
    Heap<uint32_t> entry(tiles);
    for (uint64_t t = 0; t < tiles; ++t) entry[t] = sa::kLpfNone;
    for (uint64_t k = 0; k < c; ++k)
        if (flag[k]) {
            if (entry[cand[k] / B] != sa::kLpfNone) FAIL("%s n=%llu B=%u: two entries in one tile", what, (ull)n, B);
            entry[cand[k] / B] = (uint32_t)cand[k];
        }
    std::vector<std::vector<uint32_t>> got;
    for (uint64_t t = 0; t < tiles; ++t) {
        const uint64_t base = t * B, end = std::min<uint64_t>(base + B, n);
        if (entry[t] == sa::kLpfNone) continue;
        Heap<uint32_t> a(B), b(B);
        Heap<uint8_t> f(B);
        for (uint32_t i = 0; i < B; ++i) {
            uint32_t x = B;
            if (base + i < n) {
                const uint64_t nx = sa::lz_next(base + i, lpf[base + i], n);
                if (nx < end) x = (uint32_t)(nx - base);
            }
            a[i] = x;
            f[i] = base + i == entry[t];
        }
        Heap<uint32_t>* pc = &a;
        Heap<uint32_t>* pn = &b;
        for (int k = 0; k < rounds; ++k) {
            for (uint32_t i = 0; i < B; ++i) {
                const uint32_t x = (*pc)[i];
                if (x < B) {
                    if (f[i]) f[x] = 1;
                    (*pn)[i] = (*pc)[x];
                } else {
                    (*pn)[i] = B;
                }
            }
            std::swap(pc, pn);
        }
        for (uint32_t i = 0; base + i < end; ++i)
            if (f[i]) {
                const uint64_t p = base + i;
                got.push_back({(uint32_t)p, (uint32_t)(sa::lz_next(p, lpf[p], n) - p), lpf[p] ? src[p] : sa::kLpfNone});
            }
    }
    if (got != want)
        FAIL("%s n=%llu B=%u: %llu phrases, the serial walk has %llu (or they differ)", what, (ull)n, B,
             (ull)got.size(), (ull)want.size());
    g_checks += (long)want.size() + 1;
    return true;
}

static bool check_text(const std::vector<uint8_t>& t) {
    const uint64_t n = t.size();
    Heap<uint32_t> s(n), l(n), rank(n);
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
    }
    // the definition, and the canonical source
    std::vector<uint32_t> lpf(n), src(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t best = 0;
        for (uint64_t j = 0; j < i; ++j) best = std::max(best, common(t, j, i));
        const uint64_t r = rank[i];
        uint32_t la = 0, lb = 0, va = 0, vb = 0;
        uint32_t m = l[r];
        for (uint64_t a = r; a-- > 0;) {
            if (s[a] < i) {
                la = m;
                va = s[a];
                break;
            }
            m = std::min(m, l[a]);
        }
        m = ~0u;
        for (uint64_t b = r + 1; b < n; ++b) {
            m = std::min(m, l[b]);
            if (s[b] < i) {
                lb = m;
                vb = s[b];
                break;
            }
        }
        lpf[i] = std::max(la, lb);
        src[i] = (la >= lb && la > 0) ? va : (lb > 0 ? vb : sa::kLpfNone);
        if (lpf[i] != best) FAIL("n=%llu i=%llu: the lemma gives %u, the definition %llu", (ull)n, (ull)i, lpf[i], (ull)best);
        if (lpf[i] && (src[i] >= i || common(t, src[i], i) != lpf[i]))
            FAIL("n=%llu i=%llu: source %u does not match %u bytes", (ull)n, (ull)i, src[i], lpf[i]);
        ++g_checks;
    }
    if (!check_lpf<64>(t, s, l, lpf, src) || !check_lpf<4>(t, s, l, lpf, src)) return false;
    Heap<uint32_t> hl(n), hs(n);
    for (uint64_t i = 0; i < n; ++i) {
        hl[i] = lpf[i];
        hs[i] = src[i];
    }
    for (uint32_t B : {4u, 8u, 16u})
        if (!check_parse(hl, hs, n, B, "text")) return false;
    return true;
}

// n = 2^32 - 1 with nothing behind the accessors
struct Ascending {   // SA[r] = r, lcp all 1: nothing smaller to the right of any rank
    uint64_t cnt[sa::kLpfMaxLevels];
    int n_levels;
    mutable long reads = 0;
    int levels() const { return n_levels; }
    uint64_t count(int k) const { return cnt[k]; }
    sa::LpfNode operator()(int k, uint64_t i) const {
        ++reads;
        if (i >= cnt[k]) {
            std::printf("FAIL node (%d, %llu) read\n", k, (ull)i);
            std::abort();
        }
        uint64_t first = i;
        for (int j = 0; j < k; ++j) first *= 64;
        return sa::LpfNode{(uint32_t)first, 1u};
    }
};

static bool check_large() {
    const uint64_t n = 0xFFFFFFFFull;
    if (sa::lz_next(n - 1, 0xFFFFFFFFu, n) != n || sa::lz_next(n - 1, 0, n) != n || sa::lz_next(0, 0xFFFFFFFFu, n) != n ||
        sa::lz_next(0, 0xFFFFFFFEu, n) != n - 1 || sa::lz_next(n - 2, 0, n) != n - 1 || sa::lz_next(5, 0, 6) != 6 ||
        sa::lz_next(5, 7, 100) != 12 || sa::lz_next(0xFFFFFFF0ull, 0xFFFFFFF0u, n) != n)
        FAIL("lz_next does not clamp in 64 bits");
    g_checks += 8;
    // a jump in the last tile: slots below 4096 only, values up to n
    const uint64_t base = n / 4096 * 4096, end = n;
    const auto at = [&](uint32_t k) -> uint32_t {
        if (k >= 4096) {
            std::printf("FAIL slot %u read\n", k);
            std::abort();
        }
        return (uint32_t)n;
    };
    if (sa::lz_jump((uint32_t)(n - 1), base, end, at) != (uint32_t)n || sa::lz_jump((uint32_t)n, base, end, at) != (uint32_t)n ||
        sa::lz_jump((uint32_t)base, base, end, at) != (uint32_t)n)
        FAIL("lz_jump at n = 2^32 - 1");
    g_checks += 3;
    // candidates at every 4096th position
    const uint64_t c = (n + 4095) / 4096;
    const auto cand = [&](uint64_t k) -> uint64_t {
        if (k >= c) {
            std::printf("FAIL candidate %llu read\n", (ull)k);
            std::abort();
        }
        return k * 4096;
    };
    if (sa::lz_cand_succ(cand, c, (c - 1) * 4096, n) != c - 1 || sa::lz_cand_succ(cand, c, n, n) != c ||
        sa::lz_cand_succ(cand, c, 4097, n) != c || sa::lz_cand_succ(cand, c, 0, n) != 0 || sa::lz_reach_rounds(c) != 20 ||
        sa::lz_reach_rounds(1) != 0 || sa::lz_reach_rounds(2) != 1 || sa::lz_reach_rounds(3) != 2 ||
        sa::lz_reach_rounds(n) != 32)
        FAIL("candidate arithmetic at n = 2^32 - 1");
    g_checks += 9;
    Ascending h;
    h.n_levels = sa::lpf_level_counts<64>(n, h.cnt);
    if (h.n_levels != 7 || h.cnt[1] != (1ull << 26) || h.cnt[5] != 4 || h.cnt[6] != 1) FAIL("level counts at 2^32 - 1");
    for (uint64_t r : {(uint64_t)0, (uint64_t)5, (uint64_t)4095, (uint64_t)4096, (uint64_t)123456789, n - 2, n - 1}) {
        uint32_t m = ~0u, val = 0;
        h.reads = 0;
        if (sa::lpf_walk_right<64, sa::kLpfChunk>(h, r, (uint32_t)r, m, val)) FAIL("ascending SA: a smaller value to the right of %llu", (ull)r);
        if (h.reads > (64 + sa::kLpfChunk) * 7 || (r + 1 < n && m != 1u)) FAIL("ascending SA: %ld reads from rank %llu", h.reads, (ull)r);
        m = 7;
        h.reads = 0;
        const bool f = sa::lpf_walk_left<64, sa::kLpfChunk>(h, r, (uint32_t)r, m, val);
        if (f != (r > 0) || (f && (val != r - 1 || m != 7 || h.reads > 7 * sa::kLpfChunk))) FAIL("ascending SA: left of rank %llu", (ull)r);
        // nothing at all is smaller than 0: the walk runs to rank 0
        m = 7;
        h.reads = 0;
        if (sa::lpf_walk_left<64, sa::kLpfChunk>(h, r, 0u, m, val) || h.reads > (64 + sa::kLpfChunk) * 7) FAIL("ascending SA: left walk to rank 0 from %llu", (ull)r);
        g_checks += 3;
    }
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
    // arbitrary LPF arrays: the parse stays the serial walk's
    for (int rep = 0; rep < 300; ++rep) {
        const uint64_t n = rng() % 301;
        Heap<uint32_t> lpf(n), src(n);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t k = rng() % 8;
            lpf[i] = k == 0 ? 0xFFFFFFFFu : k < 4 ? 0u : rng() % 40;
            src[i] = rng();
        }
        for (uint32_t B : {4u, 8u, 16u})
            if (!check_parse(lpf, src, n, B, "arbitrary")) return 1;
    }
    if (!check_large()) return 1;
    std::printf("ok %ld checks on %d texts\n", g_checks, texts);
    return 0;
}
