// sa_limits.h -- host-side size gates of the round-1 plan and the map of the
// context's pinned read-back words, kept free of HIP so that
// tests/cpp/limits_check.cpp can check them with g++: the gates at the
// boundaries the device code cannot be driven to in a test, the map for
// regions that share a word.
#pragma once
#include <cstdint>

namespace sa {

constexpr uint32_t kXqQueues = 8;             // per-XCD queues of the second bucket pass (sa_split.h kXq)
constexpr uint32_t kXqRegionSlack = 2048;     // per (queue, digit) sub-region slack (sa_split.h kXqSlack)
constexpr uint32_t kXqMaxDigits = 1024;       // the second pass's widest digit (10 bits)

// Items of the second pass's 8 per-XCD output regions for m suffixes: digit
// h of queue q gets tot(h)/8 + tot(h)/128 + slack (k_xq_dh), so the regions
// hold at most m + m/16 + 8 * 1024 * slack items.
constexpr uint64_t xq_region_space(uint64_t m) {
    return m + m / 16 + (uint64_t)kXqQueues * kXqMaxDigits * kXqRegionSlack;
}

// The regions are addressed with 32-bit offsets (k_split_seg<.., XQ>,
// k_bucket_starts_xq, load_items_xq): the XQ pass runs only when every
// offset fits (past ~4.02e9 suffixes queue 7 wrapped onto region 0).
constexpr bool xq_offsets_fit(uint64_t m) { return xq_region_space(m) <= 0xFFFFFFFFull; }

// sa_context::host_words, the pinned block every read-back of a few words lands in.  The entry points call each
// other on one context (hamming runs find, locate and locate's sort; MEMs matching statistics and locate; the
// FM and document listings locate's sort), so no two regions may share a word.
// Words [0, 16) mirror the device-side words[] one to one: [0..2] D, m, G; [3] kChkErrWord; [4] radix look-back
// left open; [5] the largest window; [6] local sort flags; [7] windows; [8] kAlphaBadWord; [9] a queue's digit
// outgrew its sub-region; [10] one-bucket windows; [11] kPadOverWord; [12] kPlaceErrWord (round 1:
// kUsFlagWord); [13] kPermErrWord (round 1: kRetryWord); [14] kHdrWord.
struct HostRegion {
    uint32_t at, len;   // words
    bool wide;          // read through a uint64_t*
};
constexpr uint32_t kHostWords = 4096;          // sa_context_create allocates these
constexpr int kDWord = 0;                      // words[]: distinct keys (group heads) of the set just segmented
constexpr int kMWord = 1;                      // words[]: its suffixes left unsorted
constexpr int kGWord = 2;                      // words[]: their groups
constexpr int kChkErrWord = 3;                 // words[]: the checker's error bits
constexpr int kLookbackWord = 4;               // words[]: a radix pass's look-back did not complete
constexpr int kPadOverWord = 11;               // words[]: a digit outgrew its padded segment
constexpr int kPlaceErrWord = 12;              // words[]: place_by_permutation's error bits (LCP, inverse SA)

// The regions are the rows of this table alone, one per HwId in its order: a row left out has length 0 and fails below.
enum HwId { kHwWords, kHwTotals, kHwUTotals, kHwGsInit, kHwLcpBest, kHwLcpCounts, kHwAlpha, kHwCode, kHwDistCounts, kHwTail,
            kHwLocate, kHwMem, kHwLz, kHwRepeats, kHwIbwt, kHwFmTotals, kHwFmLocate, kHwDocs, kHwHamming, kHwEdit, kHwCount };
constexpr HostRegion kHostRegions[kHwCount] = {
    {0, 16, false},        // kHwWords: the mirror of words[]
    {16, 3, false},        // kHwTotals: the segment totals of a round
    {20, 3, false},        // kHwUTotals: the totals of the unsorted set
    {24, 2, false},        // kHwGsInit: the first group starts, host to device
    {28, 2, false},        // kHwLcpBest: (length, position) of the longest repeat, 8 bytes copied out
    {32, 15, false},       // kHwLcpCounts: unresolved pairs per window (kLongRounds + 1)
    {64, 8, false},        // kHwAlpha: the 256-bit mask of the bytes present
    {320, 128, false},     // kHwCode: 256 16-bit codes
    {1024, 1024, false},   // kHwDistCounts: per-rank counts of the range-partitioned build (kDistMaxWorld)
    {2048, 16, false},     // kHwTail: the text's last kMaxK = 64 bytes
    {3072, 6, true},       // kHwLocate: total, large queries, their hits
    {3080, 6, true},       // kHwMem: candidates, skipped | total
    {3088, 2, true},       // kHwLz: z
    {3096, 4, true},       // kHwRepeats: the count, the sum of hi - lo
    {3104, 8, true},       // kHwIbwt: the kIbwtDevInfo = 4 words of info
    {3200, 257, false},    // kHwFmTotals: 256 byte totals, bwt[p]
    {3460, 10, true},      // kHwFmLocate: index?, s, n, class | total
    {3520, 4, true},       // kHwDocs: total, long queries
    {3528, 4, true},       // kHwHamming: candidates | total
    {3536, 6, true},       // kHwEdit: candidates | ends before the unique | total
};
constexpr HostRegion hw(HwId id) { return kHostRegions[id]; }

// 0: every region inside the block, no two sharing a word; 1: a 64-bit region starts at an even word, holds whole ones
constexpr bool host_regions_ok(int check) {
    for (int i = 0; i < kHwCount; ++i) {
        const HostRegion a = kHostRegions[i];
        if (check == 0 && (a.len == 0 || a.at + a.len > kHostWords)) return false;
        if (check == 1 && a.wide && (a.at % 2 || a.len % 2)) return false;
        for (int j = 0; j < i && check == 0; ++j)
            if (a.at < kHostRegions[j].at + kHostRegions[j].len && kHostRegions[j].at < a.at + a.len) return false;
    }
    return true;
}
static_assert(host_regions_ok(0), "host_words: two regions share a word, or a row of the table is missing");
static_assert(host_regions_ok(1), "host_words: a 64-bit region at an odd word");

}  // namespace sa
