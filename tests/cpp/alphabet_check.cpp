// Host check of the sampled alphabet's arithmetic (hpc_suffix_array_amd/csrc/
// sa_alpha.h) against byte-wise tests: the DNA predicate for all 256 values
// in each of the four byte lanes with the other lanes valid, and for 10^6
// random words; the byte map's marker test and the digits it leaves for
// sigma in {2, 4, 62, 127, 255} and every byte value, against the presence
// mask; the sample's layout (first and last block, at most n / 64 bytes,
// increasing blocks inside the text).  Prints "ok <cases>" or the first
// mismatch.  Built by tests/test_alphabet_proof_core.py.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sa_alpha.h"

typedef unsigned long long ull;
static long g_cases = 0;

#define FAIL(...)                         \
    do {                                  \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");                \
        return false;                     \
    } while (0)

static bool is_acgt(uint32_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }

static bool word_foreign(uint32_t w) {
    for (int i = 0; i < 4; ++i)
        if (!is_acgt((w >> (8 * i)) & 0xFFu)) return true;
    return false;
}

static bool check_dna() {
    const uint32_t letters[4] = {'A', 'C', 'G', 'T'};
    // the four letters' digits are 0..3 in this order (the pass's SWAR map)
    for (uint32_t d = 0; d < 4; ++d)
        if ((sa::dna_digits(letters[d] * 0x01010101u) & 0xFFu) != d) FAIL("digit of %c", (int)letters[d]);
    for (int lane = 0; lane < 4; ++lane)
        for (uint32_t v = 0; v < 256; ++v)
            for (uint32_t o = 0; o < 64; ++o) {   // every choice of the three other lanes' letters
                uint32_t w = 0, q = o;
                for (int i = 0; i < 4; ++i) {
                    uint32_t b = v;
                    if (i != lane) {
                        b = letters[q & 3u];
                        q >>= 2;
                    }
                    w |= b << (8 * i);
                }
                const uint32_t dig = sa::dna_digits(w);
                if ((dig & ~0x03030303u) != 0) FAIL("digits of %08x out of range", w);
                if ((sa::dna_foreign(w, dig) != 0) != !is_acgt(v)) FAIL("lane %d value %u word %08x", lane, v, w);
                ++g_cases;
            }
    std::mt19937 rng(12345);
    for (int t = 0; t < 1000000; ++t) {
        uint32_t w = rng();
        // half of the words mostly valid: random letters with up to one random byte
        if (t & 1) {
            const uint32_t r = rng();
            w = 0;
            for (int i = 0; i < 4; ++i) w |= letters[(r >> (2 * i)) & 3u] << (8 * i);
            if (r & 0x100u) w = (w & ~(0xFFu << (8 * ((r >> 9) & 3u)))) | (((r >> 16) & 0xFFu) << (8 * ((r >> 9) & 3u)));
        }
        if ((sa::dna_foreign(w, sa::dna_digits(w)) != 0) != word_foreign(w)) FAIL("random word %08x", w);
        ++g_cases;
    }
    return true;
}

// a presence mask of sigma byte values -> the pass's byte map
static bool check_generic() {
    std::mt19937 rng(777);
    const uint32_t sigmas[] = {2, 4, 62, 127, 255};
    for (uint32_t sigma : sigmas)
        for (int rep = 0; rep < 4; ++rep) {
            std::vector<uint32_t> present(256, 0);
            // rep 0: the lowest values, 1: the highest, else random ones
            for (uint32_t k = 0; k < sigma;) {
                const uint32_t b = rep == 0 ? k : rep == 1 ? 255u - k : rng() & 0xFFu;
                if (!present[b]) {
                    present[b] = 1;
                    ++k;
                }
            }
            uint32_t map[256], code = 0;
            for (uint32_t b = 0; b < 256; ++b) map[b] = sa::alpha_map_entry(present[b] ? ++code : 0u);
            if (code != sigma) FAIL("sigma %u", sigma);
            for (uint32_t b = 0; b < 256; ++b) {
                if (map[b] > 0xFFu) FAIL("entry of %u does not fit a byte", b);
                if (present[b] && map[b] >= sigma) FAIL("digit of %u", b);
                if ((map[b] == sa::kAlphaAbsent) != !present[b]) FAIL("sigma %u: marker of byte %u", sigma, b);
            }
            // every byte value in every lane beside three random bytes, and random words
            for (int t = 0; t < 4 * 256 + 20000; ++t) {
                uint32_t bytes[4];
                for (int i = 0; i < 4; ++i) bytes[i] = rng() & 0xFFu;
                if (t < 4 * 256) bytes[t >> 8] = (uint32_t)t & 0xFFu;
                uint32_t m = 0, want_digits = 0;
                bool want = false;
                for (int i = 0; i < 4; ++i) {
                    m |= map[bytes[i]] << (8 * i);
                    want |= !present[bytes[i]];
                    want_digits |= (present[bytes[i]] ? map[bytes[i]] : 0u) << (8 * i);
                }
                const uint32_t a = sa::absent_bytes(m);
                if ((a != 0) != want) FAIL("sigma %u: entries %08x", sigma, m);
                for (int i = 0; i < 4; ++i)
                    if ((((a >> (8 * i)) & 0xFFu) == 0x80u) != !present[bytes[i]] || ((a >> (8 * i)) & 0x7Fu))
                        FAIL("sigma %u: entries %08x, lane %d of %08x", sigma, m, i, a);
                if (sa::absent_to_zero(m, a) != want_digits) FAIL("sigma %u: digits of %08x", sigma, m);
                ++g_cases;
            }
        }
    return true;
}

static bool check_layout() {
    const uint64_t B = sa::kAlphaBlock;
    const uint64_t sizes[] = {1, 4095, 4096, 4097, 8192, 67649, (1ull << 26) - 1, 1ull << 26, (1ull << 26) + 4097,
                              (1ull << 30), (1ull << 30) + 1, (1ull << 31), 0xFFFFFFFFull};
    for (uint64_t n : sizes)
        for (int small = 0; small < 2; ++small) {
            const uint64_t nb = sa::alpha_text_blocks(n), ns = sa::alpha_sample_blocks(n, small != 0);
            if (ns < 1 || ns > nb) FAIL("n %llu: %llu of %llu blocks", (ull)n, (ull)ns, (ull)nb);
            if (small && ns != 1) FAIL("n %llu: the small sample is one block", (ull)n);
            if (sa::alpha_block(0, nb, ns) != 0) FAIL("n %llu: first block", (ull)n);
            if (!small && sa::alpha_block(ns - 1, nb, ns) != nb - 1) FAIL("n %llu: last block", (ull)n);
            uint64_t bytes = 0, prev = 0;
            for (uint64_t j = 0; j < ns; ++j) {
                const uint64_t k = sa::alpha_block(j, nb, ns);
                if (k >= nb || (j && k <= prev)) FAIL("n %llu: block %llu -> %llu", (ull)n, (ull)j, (ull)k);
                prev = k;
                bytes += k + 1 == nb ? n - k * B : B;
                ++g_cases;
            }
            if (bytes != sa::alpha_sample_bytes(n, small != 0)) FAIL("n %llu: bytes", (ull)n);
            if (!small && n >= (1ull << 26) && bytes > n / 64) FAIL("n %llu: %llu bytes sampled", (ull)n, (ull)bytes);
        }
    return true;
}

int main() {
    if (!check_dna() || !check_generic() || !check_layout()) return 1;
    std::printf("ok %ld\n", g_cases);
    return 0;
}
