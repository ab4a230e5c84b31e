// sa_alpha.h -- the sampled alphabet: which blocks of the text the sample
// reads (build_packed, k_alphabet_sample) and the predicates by which the
// first bucket pass proves it on every byte it stages (k_split_text).  Host-
// and device-compilable, so that tests/test_alphabet_proof_core.py can check
// them against byte-wise tests with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define SA_HD __host__ __device__ __forceinline__
#else
#define SA_HD inline
#endif

namespace sa {

// --- the sample's layout: a function of n alone ----------------------------
// Blocks of kAlphaBlock aligned bytes (the text's offsets, not its address),
// one of every kAlphaEvery: at most n / 64 bytes.  Block j of the sample is
// block alpha_block(j, nb, ns) of the text's nb blocks; j = 0 is the first
// and j = ns - 1 the last (partial) one.
constexpr uint32_t kAlphaBlock = 4096;
constexpr uint32_t kAlphaEvery = 64;

SA_HD uint64_t alpha_text_blocks(uint64_t n) { return (n + kAlphaBlock - 1) / kAlphaBlock; }

// sampled blocks (>= 2 from two text blocks up; first4k: the first block only)
SA_HD uint64_t alpha_sample_blocks(uint64_t n, bool first4k) {
    const uint64_t nb = alpha_text_blocks(n);
    if (first4k || nb <= 1) return nb ? 1 : 0;
    const uint64_t ns = n / ((uint64_t)kAlphaBlock * kAlphaEvery);
    return ns < 2 ? 2 : ns;
}

SA_HD uint64_t alpha_block(uint64_t j, uint64_t nb, uint64_t ns) {
    return ns <= 1 ? 0 : (uint64_t)(((unsigned __int128)j * (nb - 1)) / (ns - 1));
}

// bytes the sample reads
SA_HD uint64_t alpha_sample_bytes(uint64_t n, bool first4k) {
    const uint64_t nb = alpha_text_blocks(n), ns = alpha_sample_blocks(n, first4k);
    if (ns == 0) return 0;
    const uint64_t last = alpha_block(ns - 1, nb, ns);
    const uint64_t last_len = last + 1 == nb ? n - last * kAlphaBlock : kAlphaBlock;
    return (ns - 1) * kAlphaBlock + last_len;
}

// --- DNA: each byte of a word is exactly A, C, G or T -----------------------
// The pass's digit ((b >> 1) ^ (b >> 2)) & 3 maps EVERY byte to some digit
// (B like C, a like A, U and E like T): the proof rebuilds the letter from the
// digit and compares.  dig: the four digits of w, one per byte
// (dna_digits(w)); the result is non-zero when a byte of w is foreign.
SA_HD uint32_t dna_digits(uint32_t w) { return ((w >> 1) ^ (w >> 2)) & 0x03030303u; }

// byte i of the result = byte (sel's byte i, 0..3) of tab
SA_HD uint32_t select_bytes(uint32_t tab, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, tab, sel);   // selectors 0..3: the second operand's bytes
#else
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= ((tab >> (8 * ((sel >> (8 * i)) & 3u))) & 0xFFu) << (8 * i);
    return r;
#endif
}

SA_HD uint32_t dna_foreign(uint32_t w, uint32_t dig) { return w ^ select_bytes(0x54474341u /* T G C A */, dig); }

// --- any other alphabet: the byte map marks absent bytes --------------------
// The map's entry of a present byte is its dense digit (code - 1 <= 254); an
// absent byte's is kAlphaAbsent, which the pass turns into digit 0 (so that
// every bucket, cursor and item of a refuted pass stays in range).  With all
// 256 bytes present, 255 is a real digit and there is nothing to prove: the
// pass then runs without the marker test (k_split_text: alpha_bad == null).
constexpr uint32_t kAlphaAbsent = 0xFFu;

SA_HD uint32_t alpha_map_entry(uint32_t code /* dense code 1..sigma, 0 = absent */) {
    return code ? code - 1u : kAlphaAbsent;
}

// four map entries, one per byte: bit 7 of every byte that is kAlphaAbsent
SA_HD uint32_t absent_bytes(uint32_t m) { return ((m & 0x7F7F7F7Fu) + 0x01010101u) & m & 0x80808080u; }

// the entries' digits: absent bytes (a = absent_bytes(m)) become 0
SA_HD uint32_t absent_to_zero(uint32_t m, uint32_t a) { return m & ~(a | (a - (a >> 7))); }

}  // namespace sa
