/*
 * include/sa_hip.h -- extended 64-bit C ABI of libsa_hip.so.
 *
 * The reference has no 64-bit or device-resident entry point; these replace
 * what its callers do around build_suffix_array (manber_myers.c:81-133):
 *   sa_build_ex      -- host text in, host SA out (create+build of
 *                       main_sequential.c:97-109 without the int n limit,
 *                       SURVEY.md 8(b) "What the replacement exports" (2))
 *   sa_build_device  -- text already resident in HBM, SA written to HBM
 *                       (what bench.py times)
 *   sa_check[_device]-- O(n) validity check replacing is_valid_suffix_array
 *                       (manber_myers.c:184-202), SURVEY.md 8(b) (3)
 * All functions return 0 on success or a negative SA_E* code; the text of
 * the last error of the calling thread is available from sa_last_error().
 * No torch types cross this boundary: plain pointers, sizes and a stream
 * handle (hipStream_t passed as void*, NULL = the null stream).
 */
#ifndef SA_HIP_H
#define SA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_OK 0
#define SA_E_INVALID (-1)   /* bad argument (NULL pointer, width, n too large) */
#define SA_E_NOMEM (-2)     /* device or host allocation failed */
#define SA_E_HIP (-3)       /* HIP runtime error (no device, launch failure) */
#define SA_E_INTERNAL (-4)  /* internal consistency check failed */

#define SA_MAX_ROUNDS 64

/* kernel kinds timed when sa_opts.profile != 0 */
enum sa_kernel_kind {
    SA_K_INIT = 0,           /* text -> rank_1 (reference schedule) */
    SA_K_HIST_FIRST = 1,     /* digit histogram, keys generated (text/ranks) */
    SA_K_HIST_KEYS = 2,      /* digit histogram over stored keys */
    SA_K_SCAN = 3,           /* digit x chunk offset scan */
    SA_K_SCATTER_FIRST = 4,  /* stable scatter, keys generated (text/ranks) */
    SA_K_SCATTER_KEYS = 5,   /* stable scatter over stored (key, idx) */
    SA_K_HEADS = 6,          /* group-head count per chunk (reference schedule) */
    SA_K_HEADS_SCAN = 7,     /* chunk scan of head counts, D_j */
    SA_K_RERANK = 8,         /* dense rank -> rank[idx] scatter */
    SA_K_SEG_COUNT = 9,      /* heads / unsorted / group counts per chunk */
    SA_K_SEG_SCAN = 10,      /* chunk scan of those counts */
    SA_K_SEG_WRITE = 11,     /* rank + SA update, unsorted-set compaction */
    SA_K_ALPHABET = 12,      /* byte histogram of the text */
    SA_K_PACK = 13,          /* packed K-symbol keys + first digit histogram */
    SA_K_SORT_U = 14,        /* every pass of an unsorted-set (later round) sort */
    SA_K_WINDOWS = 15,       /* bucketed round 1: window starts over the bucket-sorted keys */
    SA_K_LOCAL_SORT = 16,    /* bucketed round 1: per-window LDS sort */
    SA_K_PIVOT_KEYS = 17,    /* pivot round: keys (g, rank[i + h]) and group starts */
    SA_K_PIVOT_COUNT = 18,   /* pivot round: class counts (< = > pivot) per chunk, scanned */
    SA_K_PIVOT_WRITE = 19,   /* pivot round: tied blocks out, the rest compacted */
    SA_K_COUNT = 20
};

/* first round of the packed schedule */
#define SA_ROUND1_AUTO 0      /* bucketed when n >= 2^20 and it fits, else LSD */
#define SA_ROUND1_LSD 1       /* LSD radix sort of the packed K-symbol key */
#define SA_ROUND1_BUCKETED 2  /* two bucket passes + per-window LDS sort (falls
                                 back to LSD when a window exceeds the LDS tile) */
#define SA_ROUND1_PIVOT 3     /* sa_stats.round1 only: the LSD round's keys split
                                 around the key of suffix 0, half or more of the
                                 suffixes tied to it (sa_pivot.h) */

/* doubling schedules */
#define SA_SCHEDULE_PACKED 0     /* default: first round sorts a packed K-symbol
                                    prefix; later rounds re-sort only suffixes
                                    whose group is not yet a singleton */
#define SA_SCHEDULE_REFERENCE 1  /* the reference's schedule (manber_myers.c:
                                    94-125): h = 1, 2, 4, ...; D_0 = 256; every
                                    round sorts all n (rank[i], rank[i+h]) pairs */

/* sa_opts.debug: alternative code paths the tests and A/B runs force (0 in
 * production; the library reads no environment variable that changes a
 * build).  Every combination gives the same suffix array. */
#define SA_DEBUG_NO_CMP 0x1u            /* bucketed round 1: original key1 low, not the compact one */
#define SA_DEBUG_NO_PK8 0x2u            /* bucketed round 1: key1 + position, not packed 8-byte items */
#define SA_DEBUG_NO_PAD 0x4u            /* bucketed round 1: exact digit totals, not sampled padded segments */
#define SA_DEBUG_PAD_OVERFLOW 0x8u      /* forced overflow of the padded round-1 layouts, which then re-run exactly:
                                           one GPU: padded first-pass segments with no slack; range builds
                                           (sa_dist_round1): striped record regions of half their share, the
                                           round re-runs with the counting record scan */
#define SA_DEBUG_NO_FAST32 0x10u        /* local sort: measured-span kernel, not the fixed-span 32-bit one */
#define SA_DEBUG_NO_PIVOT 0x20u         /* later rounds: full sorts, never the three-way pivot split */
#define SA_DEBUG_PERM_ALWAYS 0x40u      /* reference schedule: permutation re-rank at every n */
#define SA_DEBUG_NO_XQ 0x80u            /* bucketed round 1: second pass into one region (one ticket), not per-XCD
                                           queues and regions */
#define SA_DEBUG_XQ_OVERFLOW 0x100u     /* per-XCD second pass with sub-regions of exactly 1/8 of each digit: a queue
                                           overflows and the round re-runs with the one-region pass */
#define SA_DEBUG_NO_KEY1_ROUND 0x400u   /* the first round after a sparse bucketed round 1 takes its keys' ranks by
                                           the sample search (RankLookup), not as key1 rebuilt from the text */
#define SA_DEBUG_NO_TIED 0x200u         /* pivot rounds: tied blocks through the sorted output and segments(), not
                                           written straight to the next unsorted set (sa_pivot.h) */
#define SA_DEBUG_NO_EONLY 0x800u        /* non-power-of-two alphabets: keep the compact key1 layout (and 12-byte
                                           first-pass items) instead of the E-only layout that packs them */
#define SA_DEBUG_EONLY 0x1000u          /* bucketed round 1: the E-only key1 layout whenever the text's tail allows
                                           it (tests; production takes it only for packed non-power-of-two items) */
#define SA_DEBUG_FAST32_SMALL 0x2000u   /* local sort: the fixed-span 32-bit kernel whenever the key span allows it,
                                           whatever the average bucket size (tests: reaches it below 2^28 suffixes;
                                           windows of several buckets still take the measured-span kernel) */
#define SA_DEBUG_NO_ROUND2_FUSED 0x4000u /* one GPU: round 2 through the compacted unsorted set and segments(), not
                                           finished from the local sort's staging by k_round2_windows (A/B runs, tests) */
#define SA_DEBUG_LS_ONE_WG 0x8000u      /* local sort: the fixed-span 32-bit kernel launched with one workgroup, so
                                           every listed window passes through it in ticket order (tests of the
                                           window-to-window hand-over at sizes an oracle sorts; phase times of one
                                           workgroup); the plan, the windows and the statistics stay the same */
#define SA_DEBUG_NO_ALPHA_SAMPLE 0x10000u /* packed schedule: the alphabet always from the pass over the whole text,
                                           never from a sample that the first bucket pass proves (A/B runs; callers
                                           who want no speculative work: a text with a symbol in none of the sampled
                                           blocks pays a wasted first and second pass before the exact re-run) */
#define SA_DEBUG_ALPHA_SAMPLE_SMALL 0x20000u /* the sampled alphabet at any n, its sample the text's first 4096 bytes
                                           only (tests: both outcomes at sizes an oracle sorts) */
#define SA_DEBUG_BB17 0x40000u          /* bucketed round 1 on one GPU: at least 17 bucket bits, whatever the size
                                           (tests: the second bucket pass's 9-bit digit, which production takes
                                           from 2^29 suffixes, at sizes an oracle sorts; never fewer bits than
                                           the size gives; the range-partitioned build ignores it) */
#define SA_DEBUG_BB18 0x80000u          /* the same with 18 bucket bits (the 10-bit digit: production from 2^30
                                           suffixes); wins over SA_DEBUG_BB17 when both are set */

/* sa_stats.alphabet */
#define SA_ALPHABET_EXACT 0    /* from a pass over the whole text */
#define SA_ALPHABET_SAMPLED 1  /* from a sample, proven by the first bucket pass */
#define SA_ALPHABET_REFUTED 2  /* a sample the first bucket pass refuted: the build ran again with the exact one */

typedef struct {
    int32_t profile;        /* 1: time every launch with HIP events */
    int32_t schedule;       /* SA_SCHEDULE_* */
    int32_t init_chars;     /* packed schedule: symbols in the first key, 0 = auto */
    int32_t radix;          /* 0: single-pass radix (decoupled look-back, default);
                               1: reduce-then-scan radix (3 kernels per pass) */
    int32_t round1;         /* SA_ROUND1_* (packed schedule, onesweep radix) */
    uint32_t debug;         /* SA_DEBUG_* flags (0 = production paths) */
    int32_t span_extra;     /* debug: bits added to the local sort's fixed key span
                               (its windows all take the measured-span retry) */
    int32_t tune;           /* A/B shapes, 0 = defaults: bits 0-7 the reference
                               schedule's widest LSD digit (8..10), bits 8-15 the
                               first bucket pass's cursor stripes (1, 2, 4, 8),
                               16-19 local-sort variants, 20-23 checker level-1
                               bins / persistent split, 24-27 = 1 the persistent
                               re-rank split, 28 no 32-bit rolling (12-byte
                               first-pass items), 29 window-order local-sort
                               rows (no chunk rows), 30 LCP by the random gather
                               (no permutations) */
} sa_opts;

typedef struct {
    int32_t rounds;                      /* doubling rounds executed */
    int32_t n_kinds;                     /* = SA_K_COUNT */
    double total_ms;                     /* build time on the stream (HBM in -> HBM out) */
    double h2d_ms, d2h_ms;               /* sa_build_ex only: PCIe copies */
    double round_ms[SA_MAX_ROUNDS];      /* per doubling round */
    uint64_t distinct[SA_MAX_ROUNDS];    /* D_j: distinct h-prefix groups after round j */
    int32_t passes[SA_MAX_ROUNDS];       /* radix passes in round j */
    uint64_t sorted_n[SA_MAX_ROUNDS];    /* suffixes (re-)sorted in round j */
    uint64_t prefix_len[SA_MAX_ROUNDS];  /* h after round j (prefix length sorted) */
    int32_t schedule;                    /* SA_SCHEDULE_* used */
    int32_t init_chars;                  /* K of the packed schedule */
    int32_t sigma;                       /* distinct symbols in the text */
    int32_t sparse_ranks;                /* 1: round-1 ranks kept for unsorted suffixes only */
    int32_t round1;                      /* SA_ROUND1_LSD, _BUCKETED or _PIVOT: first round taken */
    int32_t largest_window;              /* bucketed round 1: largest window (suffixes) */
    uint64_t model_bytes;                /* SURVEY.md 8(d)'s model of the REFERENCE-shaped schedule (12-B records
                                            through P_j LSD passes per round), summed; not the bytes of the
                                            packed schedule (round_bytes / kern_bytes are) */
    double kern_ms[SA_K_COUNT];          /* profile only */
    uint64_t kern_launches[SA_K_COUNT];  /* profile only */
    uint64_t kern_bytes[SA_K_COUNT];     /* algorithmic bytes moved per kind */
    int32_t round1_segments;             /* bucketed round 1: 0 exact digit totals, 1 sampled padded segments,
                                            2 padded segments overflowed and the round ran again exactly;
                                            range builds: 3 records by one striped text scan, 4 a record
                                            stripe overflowed and the round ran again with the counting scan */
    int32_t round1_layout;               /* bucketed round 1: bit 0 compact key1 low (BucketSpec.cmp),
                                            bit 1 packed 8-byte first-pass items (PK8), bit 2 the second
                                            pass by per-XCD queues and regions (XQ), bit 3 the E-only
                                            key1 low (no end bit; non-power-of-two alphabets' PK8),
                                            bits 4-7 the second pass's digit bits hb (7..10; bucket bits - 8
                                            on one GPU) */
    uint64_t round_bytes[SA_MAX_ROUNDS]; /* algorithmic bytes of the kernels launched in round j (the kern_bytes
                                            added between its boundaries; the schedule actually run) */
    int32_t round1_windows[4];           /* bucketed round 1, the local sort's first launch: [0] non-empty windows,
                                            [1] one-bucket windows sorted by the fixed-span kernel, [2] windows
                                            sorted again with their measured span (several buckets, or keys
                                            clustered in one sub-bucket), [3] skewed windows (LSD kernel) */
    int32_t alphabet;                    /* SA_ALPHABET_*: where the dense codes came from (packed schedule) */
} sa_stats;

typedef struct sa_context sa_context;

/* Device workspace for texts of up to max_n symbols on `device`. */
int sa_context_create(int device, uint64_t max_n, sa_context** out);
/* The debug / tune fields of opts (NULL: defaults) for the calls on ctx that
 * take no sa_opts -- the range-partitioned build's sa_dist_* phases;
 * sa_build_device applies its own opts. */
int sa_context_set_debug(sa_context* ctx, const sa_opts* opts);
void sa_context_destroy(sa_context* ctx);
/* bytes of device memory a context for max_n needs */
uint64_t sa_workspace_bytes(uint64_t max_n);

/* d_text: n bytes in device memory; d_sa: n uint32 in device memory.
 * n <= 2^32 - 1.  Enqueued on `stream`; returns after the SA is complete
 * (one 4-byte D_j read-back per round synchronises the stream). */
int sa_build_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, uint32_t* d_sa,
                    void* stream, const sa_opts* opts, sa_stats* stats);

/* Host in, host out.  sa_width is 4 (int32/uint32) or 8 (int64). */
int sa_build_ex(const uint8_t* text, uint64_t n, void* sa_out, int sa_width,
                const sa_opts* opts, sa_stats* stats);

/* O(n) check on the GPU: 1 valid, 0 invalid, <0 error. */
int sa_check_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                    void* stream);
int sa_check(const uint8_t* text, uint64_t n, const void* sa, int sa_width);

/* LCP array and longest repeated substring on the GPU (replaces
 * build_lcp_array, manber_myers.c:135-157, and the lcp scan of
 * find_longest_repeated_substring, :159-182).  d_lcp[0] = 0 and
 * d_lcp[r] = lcp(SA[r-1], SA[r]) (n uint32 in device memory, may not alias
 * d_sa).  lrs_len / lrs_pos (optional) receive the first r >= 1 with the
 * strictly largest lcp: its length and SA[r] (0, 0 when nothing repeats).
 * d_lcp must be 16-byte aligned: PHI and the final LCP are placed into it by
 * the coalesced permutation, which stores 16 bytes at a time (nothing past
 * d_lcp[n - 1] is written); a misaligned d_lcp is SA_E_INVALID, "d_lcp must
 * be 16-byte aligned", before any launch.
 * Precondition: d_sa is a valid suffix array of the text (sa_check_device);
 * it is not checked here.  Synchronises `stream` before returning. */
int sa_lcp_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint32_t* d_lcp,
                  uint64_t* lrs_len, uint64_t* lrs_pos, void* stream);
/* Host in, host out: sa and lcp_out have width sa_width (4 or 8). */
int sa_lcp(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* lcp_out, uint64_t* lrs_len,
           uint64_t* lrs_pos);

/* ---- batched exact-match search over a built suffix array ---------------
 * (the reference has no search; csrc/sa_find.h).  Order is the builder's:
 * unsigned bytes, end of string smallest.  Pattern q is the m = off[q+1] -
 * off[q] bytes at pat + off[q]; its interval [lo, hi) holds the SA positions
 * r with SA[r] + m <= n and text[SA[r] .. SA[r] + m) equal to it.  A suffix
 * shorter than m that is a proper prefix of the pattern sorts below it; when
 * nothing matches lo == hi is the insertion point.  The empty pattern gives
 * [0, n), n == 0 gives [0, 0), m > n an empty interval.  Binary-safe: 0x00
 * and 0xFF are ordinary bytes, lengths are explicit.  The count is hi - lo,
 * the occurrences are SA[lo .. hi) in SA order (not text order). */

/* flags: 0 auto (patterns of up to SA_FIND_LANE_MAX bytes by one lane each,
 * longer ones by one wavefront each), SA_FIND_LANE one query per lane for
 * every pattern, SA_FIND_WAVE one query per wavefront for every pattern
 * (tests, A/B). */
#define SA_FIND_LANE 1u
#define SA_FIND_WAVE 2u
#define SA_FIND_LANE_MAX 3584   /* the measured crossover of the two kernels */

/* d_text: n bytes, d_sa: n uint32, d_pat: pat_bytes bytes, d_pat_off: nq + 1
 * uint64, d_lo / d_hi: nq uint32, all in device memory; n <= 2^32 - 1.
 * Asynchronous on `stream` (no host wait, no workspace); SA_OK without a
 * launch when nq == 0.
 * Preconditions: d_sa is a valid suffix array of the text, and the offsets
 * are non-decreasing and end at or below pat_bytes.  When they do not hold
 * the results are unspecified, but no load leaves the three buffers: an
 * SA[r] >= n reads as the empty suffix, offsets are clamped to pat_bytes and
 * a decreasing pair is the empty pattern. */
int sa_find_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                   const uint8_t* d_pat, uint64_t pat_bytes, const uint64_t* d_pat_off /* nq+1 */,
                   uint64_t nq, uint32_t* d_lo, uint32_t* d_hi, uint32_t flags, void* stream);
/* Host in, host out: sa has width sa_width (4 or 8; width-8 entries outside
 * [0, n) are SA_E_INVALID), pat_off holds nq + 1 non-decreasing offsets into
 * pat (SA_E_INVALID otherwise).  Allocates, uses and frees device buffers. */
int sa_find(const uint8_t* text, uint64_t n, const void* sa, int sa_width,
            const uint8_t* pat, const uint64_t* pat_off, uint64_t nq,
            uint64_t* lo_out, uint64_t* hi_out);
/* sa_find with the flags of sa_find_device (tests, A/B) */
int sa_find_ex(const uint8_t* text, uint64_t n, const void* sa, int sa_width,
               const uint8_t* pat, const uint64_t* pat_off, uint64_t nq,
               uint64_t* lo_out, uint64_t* hi_out, uint32_t flags);

/* ---- longest-match queries and matching statistics ----------------------
 * (csrc/sa_match.h).  Order and byte handling are sa_find's.  For a query P
 * of m bytes against the n bytes of the text, len is the largest l <= m for
 * which P[0 .. l) occurs in the text, and [lo, hi) is the sa_find interval of
 * P[0 .. len): an occurrence of the match is SA[lo], all of them are
 * SA[lo .. hi).  len == m gives exactly what sa_find gives for P; len == 0
 * gives [0, n) (m == 0, or a first byte the text does not hold); n == 0 gives
 * len 0 and [0, 0).
 * The batch form takes nq patterns as sa_find does.  The sliding form takes
 * one string of m bytes and answers for each of its positions i the query
 * string[i .. min(m, i + max_len)) (max_len == 0: to the string's end): with
 * max_len == 0 that is the matching statistics of the string against the
 * text, m entries in each output.
 * d_lo / d_hi (lo_out / hi_out) are both given or both NULL; both NULL asks
 * for the lengths only and skips the two bound searches; one of them NULL is
 * SA_E_INVALID.
 * flags: 0, SA_FIND_LANE or SA_FIND_WAVE.  0 splits the batch form's patterns
 * by length at SA_FIND_LANE_MAX as sa_find does; for the sliding form, whose
 * positions all have one cap, 0 takes the lane kernel when no query can be
 * longer than SA_FIND_LANE_MAX bytes (1 <= max_len <= SA_FIND_LANE_MAX, or
 * m <= SA_FIND_LANE_MAX) and the wave kernel otherwise.
 * The device forms are asynchronous on `stream` (no host wait, no workspace)
 * and return SA_OK without a launch when there are no queries; n <= 2^32 - 1;
 * outputs are uint32.  Preconditions and what holds without them: as for
 * sa_find_device (results unspecified, no load leaves the buffers, every
 * search ends).  The host forms allocate, use and free device buffers and
 * check their arguments as sa_find does. */
int sa_match_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                    const uint8_t* d_pat, uint64_t pat_bytes, const uint64_t* d_pat_off /* nq+1 */,
                    uint64_t nq, uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi, uint32_t flags, void* stream);
int sa_matching_stats_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                             const uint8_t* d_query, uint64_t m, uint64_t max_len /* 0 = none */,
                             uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi /* m entries each */,
                             uint32_t flags, void* stream);
int sa_match(const uint8_t* text, uint64_t n, const void* sa, int sa_width,
             const uint8_t* pat, const uint64_t* pat_off, uint64_t nq,
             uint64_t* len_out, uint64_t* lo_out, uint64_t* hi_out, uint32_t flags);
int sa_matching_stats(const uint8_t* text, uint64_t n, const void* sa, int sa_width,
                      const uint8_t* query, uint64_t m, uint64_t max_len,
                      uint64_t* len_out, uint64_t* lo_out, uint64_t* hi_out, uint32_t flags);

/* ---- Burrows-Wheeler transform and inverse suffix array -----------------
 * (csrc/sa_bwt.h).  Order: the builder's (unsigned bytes, end of string
 * smallest).  For a text of n bytes and its suffix array SA:
 *   bwt[r] = text[SA[r] - 1] where SA[r] > 0, and bwt[r] = text[n - 1] at the
 *   one rank with SA[r] == 0.  That rank is the primary index (= ISA[0]).  The
 *   output is n bytes, a permutation of the text's bytes; for a text that ends
 *   in a unique smallest byte it is the classical BWT of the text's rotations.
 *   (The (n+1)-row form of text$ is: text[n - 1] first, then these n bytes
 *   with the primary row replaced by $, primary index + 1: INTEGRATION.md.)
 *   runs      the number of maximal runs of equal bytes in bwt[0, n): 0 for
 *             n == 0, 1 for a text of one symbol.
 *   counts[c] the occurrences of byte c in bwt (= in the text).
 *   isa[SA[r]] = r.
 * Statistics are SA_BWT_STATS uint64 words: [0] primary, [1] runs, [2 + c]
 * the count of byte c. */
#define SA_BWT_STATS 258

/* d_text: n bytes, d_sa: n uint32, d_bwt: n bytes, d_stats: SA_BWT_STATS
 * uint64 or NULL, all in device memory; n <= 2^32 - 1.  Asynchronous on
 * `stream` (no host wait, no context, no workspace).  Checked before any HIP
 * call: a NULL d_text, d_sa or d_bwt with n > 0, d_bwt == d_text or d_bwt ==
 * d_sa, and n too large are SA_E_INVALID.  n == 0 is SA_OK without a launch
 * (d_stats, if given, is zeroed).
 * d_bwt may have any byte alignment; exactly d_bwt[0, n) is written.  With
 * d_stats == NULL no histogram or run work is done (another kernel
 * instantiation); with d_stats every call zeroes the words itself on the
 * stream, so two calls in a row give the same numbers.
 * Precondition: d_sa is a valid suffix array of the text.  When it is not,
 * the bytes and statistics are unspecified, but no load leaves d_text[0, n)
 * or d_sa[0, n): an entry >= n is clamped, never dereferenced, and the
 * reported primary lies in [0, n]. */
int sa_bwt_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, uint8_t* d_bwt,
                  uint64_t* d_stats /* SA_BWT_STATS words in device memory, or NULL */, void* stream);
/* Host in, host out: sa has width sa_width (4 or 8; a width-8 entry outside
 * [0, n) is SA_E_INVALID before any device work).  Allocates, uses and frees
 * device buffers.  n == 0 is SA_OK without a device, stats_out zeroed. */
int sa_bwt(const uint8_t* text, uint64_t n, const void* sa, int sa_width, uint8_t* bwt_out,
           uint64_t* stats_out /* SA_BWT_STATS words, or NULL */);

/* d_isa[d_sa[r]] = r for r < n, by the coalesced permutation of the LCP path
 * (workspace of ctx).  d_isa: exactly n uint32 in device memory, 16-byte
 * aligned (the placement stores 16 bytes at a time; nothing past d_isa[n - 1]
 * is written), not d_sa; a misaligned or aliasing d_isa is SA_E_INVALID.
 * Synchronises `stream` before returning.  A d_sa that is not a permutation
 * of [0, n) (a hole, a duplicate, an entry out of range) is SA_E_INVALID,
 * "not a permutation" in sa_last_error().  n == 0 is SA_OK. */
int sa_inverse_device(sa_context* ctx, uint64_t n, const uint32_t* d_sa, uint32_t* d_isa, void* stream);
/* Host in, host out: sa and isa_out have width sa_width (4 or 8; width-8
 * entries outside [0, n) are SA_E_INVALID before any device work). */
int sa_inverse(const void* sa, uint64_t n, int sa_width, void* isa_out /* width sa_width */);

/* ---- LF-mapping and inverse Burrows-Wheeler transform ---------------------
 * (csrc/sa_ibwt.h).  The BWT convention above: n bytes, no sentinel, and the
 * primary index p < n, the rank with bwt[p] = text[n - 1].
 *   LF        order the rows p, 0, 1, .., p - 1, p + 1, .., n - 1 and sort them
 *             stably by their byte bwt[r]: LF[r] is where row r lands.  With
 *             C[c] = the bytes below c and last = bwt[p]: LF[p] = C[last], and
 *             for r != p, LF[r] = C[c] + [c == last] + #{k < r, k != p,
 *             bwt[k] == c}, c = bwt[r].  For a genuine BWT, LF[ISA[i]] =
 *             ISA[i - 1] (i >= 1) and LF[p] = ISA[n - 1]: the rank of the
 *             suffix one position to the left.  For any bytes and any p < n it
 *             is a permutation of [0, n).
 *   inverse   r_0 = LF[p], text[n - 1] = bwt[p]; for k = 1 .. n - 1:
 *             text[n - 1 - k] = bwt[r_{k-1}], r_k = LF[r_{k-1}], SA[r_k] =
 *             n - 1 - k.  (bwt, p) is the BWT of a text, which is then unique,
 *             exactly when this chain meets p for the first time at step
 *             n - 1 (LF is one cycle of n ranks).  Anything else is
 *             SA_E_INVALID, "not a BWT" in sa_last_error(), with the outputs
 *             untouched: never a hang, never a load outside the buffers.
 * Info words of the inverse, SA_IBWT_INFO uint64: [0] the splitters of the list
 * ranking (about n / 64 + 1), [1] the longest stretch of the chain between two
 * splitters (the longest dependent walk of a lane), [2] the steps from r_0
 * until p: n - 1 for a BWT, fewer when the chain closed early. */
#define SA_IBWT_INFO 3

/* d_bwt: n bytes at any alignment, d_lf: n uint32, in device memory; n <= 2^32
 * - 1.  Asynchronous on `stream`: no host wait (ctx names the device).
 * Temporaries are stream-ordered, n / 32 bytes.  Checked before any HIP call,
 * each SA_E_INVALID: a NULL ctx; n too large; with n > 0 a NULL d_bwt or d_lf,
 * primary >= n, d_lf == d_bwt, a d_lf that is not 4-byte aligned.  n == 0 is
 * SA_OK without a launch.  Exactly d_lf[0, n) is written. */
int sa_lf_device(sa_context* ctx, const uint8_t* d_bwt, uint64_t n, uint64_t primary, uint32_t* d_lf, void* stream);
/* d_text: n bytes at any alignment, exactly d_text[0, n) is written; d_sa: n
 * uint32 or NULL (the suffix array comes out of the same walk).  Host waits
 * per call: one (the info words, after everything is enqueued; `stream` is
 * synchronised on return).  Temporaries are stream-ordered, about 4.5 n bytes
 * (LF itself is 4 n of them).  Checked before any HIP call, each
 * SA_E_INVALID: a NULL ctx; n too large; with n > 0 a NULL d_bwt or d_text,
 * primary >= n, d_text == d_bwt, d_sa == d_bwt or d_text, a d_sa that is not
 * 4-byte aligned.  n == 0 is SA_OK without a device, info zeroed.  On "not a
 * BWT" info is filled and neither d_text nor d_sa is written. */
int sa_ibwt_device(sa_context* ctx, const uint8_t* d_bwt, uint64_t n, uint64_t primary, uint8_t* d_text,
                   uint32_t* d_sa /* or NULL */, uint64_t* info /* host, SA_IBWT_INFO words, or NULL */, void* stream);
/* Host in, host out: lf_out and sa_out have `width` bytes per entry (4 or 8).
 * Checked before any device work: the width, n, NULL pointers with n > 0,
 * primary >= n, outputs that alias an input.  n == 0 is SA_OK without a
 * device.  They allocate, use and free device buffers.  sa_ibwt_ex is sa_ibwt
 * with the info words (zeroed first). */
int sa_lf(const uint8_t* bwt, uint64_t n, uint64_t primary, void* lf_out, int width);
int sa_ibwt(const uint8_t* bwt, uint64_t n, uint64_t primary, uint8_t* text_out, void* sa_out /* or NULL */,
            int sa_width);
int sa_ibwt_ex(const uint8_t* bwt, uint64_t n, uint64_t primary, uint8_t* text_out, void* sa_out /* or NULL */,
               int sa_width, uint64_t* info /* SA_IBWT_INFO words, or NULL */);

/* ---- FM-index: backward-search count and sampled locate --------------------
 * (csrc/sa_fm.h).  An index over (bwt, primary) in the convention above that
 * answers count and locate with neither the text nor the suffix array in
 * memory: about 1.25 n bytes without samples, 1.5625 n with sa_sample = 32.
 * With last = bwt[p], C[c] = the bytes below c in the BWT, base[c] = C[c] +
 * [c == last], occ(c, r) = #{k < r : bwt[k] == c} and occ'(c, r) = occ(c, r) -
 * [c == last and r > p]:
 *   count     P[0, m): lo = C[c], hi = C[c + 1] for c = P[m - 1], then for c =
 *             P[m - 2] .. P[0] while lo < hi: lo = base[c] + occ'(c, lo), hi =
 *             base[c] + occ'(c, hi).  When the pattern occurs, [lo, hi) is
 *             exactly sa_find's interval.  When it does not, the answer is
 *             lo == hi == 0: NOT sa_find's insertion point.  The empty pattern
 *             gives [0, n).
 *   locate    row r is marked iff SA[r] % sa_sample == 0 and sample[rank1(r)] =
 *             SA[r] / sa_sample; SA[r] = sa_sample * sample[rank1(q)] + k for
 *             the first marked q = LF^k[r], k < sa_sample, LF[r] = base[bwt[r]] +
 *             occ'(bwt[r], r).
 * The index is one position-independent byte buffer (offsets, never pointers)
 * that may be copied, written to disk and read back at any 16-byte aligned
 * address: a 4096-byte header, rank blocks of [cols x uint32 counts][R BWT
 * bytes] with (cols, R) = (4, 64) for up to 4 distinct bytes, (16, 256) for up
 * to 16, (256, 4096) otherwise, and with samples one mark bit per row (64-bit
 * words, per-word and per-tile counts) and ceil(n / sa_sample) uint32 samples.
 * Info words of the build, SA_FM_INFO uint64: [0] sigma, the distinct bytes,
 * [1] the class 0 / 1 / 2, [2] the bytes of the index (<= sa_fm_index_bytes),
 * [3] the samples. */
#define SA_FM_INFO 4
#define SA_FM_MAX_SAMPLE 4096

/* Pure host arithmetic: the largest of the three classes' sizes, so that the
 * caller allocates before sigma is known.  sa_sample == 0: no locate.  For
 * sa_sample = 32 and n >= 2^20 it is at most 1.6 n + 64 KiB. */
uint64_t sa_fm_index_bytes(uint64_t n, uint32_t sa_sample);

/* d_bwt: n bytes at any alignment; d_sa: the n uint32 of the suffix array, NULL
 * iff sa_sample == 0; d_index: index_bytes bytes, 16-byte aligned; all in device
 * memory; n <= 2^32 - 1, sa_sample 0 or 1 .. SA_FM_MAX_SAMPLE.  Host waits
 * per call: one (the byte counts: sigma decides the class); what follows is
 * enqueued on `stream` and not waited for.  Temporaries are stream-ordered,
 * n / 32 bytes.  Checked before any HIP call, each SA_E_INVALID with its own
 * message: a NULL ctx; n too large; sa_sample above SA_FM_MAX_SAMPLE; a NULL or
 * misaligned d_index; index_bytes below sa_fm_index_bytes(n, sa_sample); with
 * n > 0 a NULL d_bwt, primary >= n, sa_sample > 0 with a NULL d_sa or the
 * reverse, a d_sa that is not 4-byte aligned, d_index == d_bwt or d_sa.
 * n == 0 is SA_OK with a valid empty index.  d_sa is trusted to be the suffix
 * array: one that is not gives an index whose locate answers are wrong, never a
 * store outside d_index. */
int sa_fm_build_device(sa_context* ctx, const uint8_t* d_bwt, uint64_t n, uint64_t primary,
                       const uint32_t* d_sa /* NULL iff sa_sample == 0 */, uint32_t sa_sample, void* d_index,
                       uint64_t index_bytes, uint64_t* info /* host, SA_FM_INFO words, or NULL */, void* stream);
/* Patterns and results as sa_find_device's: pattern q is bytes d_pat_off[q] ..
 * d_pat_off[q + 1] of d_pat, the offsets clamped to pat_bytes and a decreasing
 * pair the empty pattern; [d_lo[q], d_hi[q]) uint32.  Asynchronous on `stream`:
 * no host wait, no context, no workspace; SA_OK without a launch when nq == 0.
 * The kernel reads the header itself: when the magic, the version, n or a
 * section's extent does not fit index_bytes every query answers (0, 0); every
 * computed row is clamped to n, so no load leaves d_index[0, index_bytes)
 * whatever the bytes are, and every search ends after m steps.  Checked before
 * any HIP call (SA_E_INVALID): a NULL pointer, a d_index that is not 16-byte
 * aligned, nq too large. */
int sa_fm_count_device(const void* d_index, uint64_t index_bytes, const uint8_t* d_pat, uint64_t pat_bytes,
                       const uint64_t* d_pat_off, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi, void* stream);
/* sa_locate_device with the index in place of (n, d_sa): d_off, d_pos,
 * max_hits, SA_LOCATE_SA_ORDER, the sizing call (d_pos NULL or *total >
 * pos_cap) and pos_cap mean the same, pos[off[q] .. off[q + 1]) = SA[lo[q] ..
 * lo[q] + c[q]) sorted ascending.  A group of 1 / 4 / 64 lanes (by class) per
 * hit resolves SA[row] by the walk above, bounded at sa_sample steps; on a
 * corrupt index the result is clamped below n.  The hits are materialised (4
 * bytes each, stream-ordered) and sorted per query by sa_locate_device's
 * kernels.  Host waits: one for the total and the header's words, then
 * sa_locate_device's own, or one at the end with SA_LOCATE_SA_ORDER.
 * SA_E_INVALID: what is no index ("not an FM-index"), an index built with
 * sa_sample == 0 ("no samples"), a total above 2^32 - 1 ("cap it with
 * max_hits"); and before any HIP call a NULL ctx, d_index, d_lo, d_hi, d_off
 * or total, a misaligned d_index, nq too large, unknown flags. */
int sa_fm_locate_device(sa_context* ctx, const void* d_index, uint64_t index_bytes, const uint32_t* d_lo,
                        const uint32_t* d_hi, uint64_t nq, uint64_t max_hits, uint32_t flags,
                        uint64_t* d_off /* nq + 1 */, uint32_t* d_pos /* may be NULL */, uint64_t pos_cap,
                        uint64_t* total, void* stream);
/* Host in, host out, over the staging of the other host forms; they allocate,
 * use and free device buffers.  sa_fm_build: sa has sa_width (4 or 8) bytes per
 * entry, NULL iff sa_sample == 0; index_out holds index_bytes >=
 * sa_fm_index_bytes(n, sa_sample) bytes, of which info[2] are written; n == 0
 * writes the empty index without a device.  sa_fm_count and sa_fm_locate check
 * the header on the host, SA_E_INVALID "not an FM-index" (index_bytes below
 * the header, a wrong magic or version, a section that ends past index_bytes);
 * lo_out / hi_out are uint64; sa_fm_locate fills off_out on the host as
 * sa_locate does, rejects lo > hi or hi > n, and writes pos_out with pos_width
 * (4 or 8) bytes per entry.  Over an empty index both return without a
 * device. */
int sa_fm_build(const uint8_t* bwt, uint64_t n, uint64_t primary, const void* sa /* NULL iff sa_sample == 0 */,
                int sa_width, uint32_t sa_sample, void* index_out, uint64_t index_bytes,
                uint64_t* info /* SA_FM_INFO words, or NULL */);
int sa_fm_count(const void* index, uint64_t index_bytes, const uint8_t* pat, const uint64_t* pat_off, uint64_t nq,
                uint64_t* lo_out, uint64_t* hi_out);
int sa_fm_locate(const void* index, uint64_t index_bytes, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                 uint64_t max_hits, uint32_t flags, uint64_t* off_out /* nq + 1 */, void* pos_out, int pos_width,
                 uint64_t pos_cap);

/* ---- batched locate: sorted hit lists in CSR form ------------------------
 * (csrc/sa_locate.h).  Inputs are a suffix array of n entries and nq SA
 * intervals [lo[q], hi[q]) -- what sa_find or sa_match return.  With
 *   c[q] = min(hi[q] - lo[q], max_hits)      (max_hits == 0: no cap)
 * the output is off[0] = 0, off[q + 1] = off[q] + c[q] (nq + 1 uint64; the
 * total is off[nq]) and pos[off[q] .. off[q + 1]) = SA[lo[q] .. lo[q] + c[q]),
 * sorted ascending.  A capped query therefore returns the FIRST max_hits hits
 * IN SA ORDER, then sorted: deterministic, but not the max_hits smallest
 * positions.  With SA_LOCATE_SA_ORDER the sort is skipped and the slices are
 * concatenated as they lie in the SA.  The text is never read.  Queries may
 * overlap or repeat, so the total may exceed n: offsets and every index into
 * pos are 64-bit.
 * A query with c[q] <= SA_LOCATE_TILE is sorted in LDS together with the
 * other queries of its output tile; a longer one goes through the context's
 * radix sort.  The class is decided on the capped count. */
#define SA_LOCATE_SA_ORDER 1u      /* positions in SA order, not sorted */
#define SA_LOCATE_SMALL_CHUNKS 2u  /* tests: the large class sorted in chunks of 2^14 hits (production: 2^28) */
#define SA_LOCATE_TILE 2048        /* output slots per tile = the largest query of the small class */

/* d_sa: n uint32, d_lo / d_hi: nq uint32, d_off: nq + 1 uint64, d_pos: pos_cap
 * uint32 or NULL, all in device memory; n and nq <= 2^32 - 1.
 * Always fills d_off and *total.  Positions are written only when d_pos is
 * not NULL and *total <= pos_cap; otherwise the call returns SA_OK with
 * *total set and touches nothing in d_pos: the sizing call, after which the
 * caller allocates and calls again.  Exactly d_pos[0, total) and d_off[0, nq]
 * are written; d_pos may have any 4-byte alignment (a view such as pos + 1).
 * Synchronises `stream`: one host wait per call when no query is large (or
 * nothing is written); with large queries one more per chunk of 2^28 large
 * hits (the radix sort's own), one when there are several chunks, and one at
 * the end.  Temporaries are stream-ordered allocations (SA_E_NOMEM when one
 * fails); the radix sort grows the context's workspace to the chunk.
 * Checked before any HIP call (SA_E_INVALID): a NULL ctx, d_sa, d_lo, d_hi,
 * d_off or total, n or nq too large, d_pos == d_sa, unknown flags.  nq == 0
 * gives off[0] = 0 and total 0 without a launch.
 * Precondition: lo <= hi <= n.  An interval that breaks it counts as empty,
 * and no load leaves d_sa[0, n), d_lo[0, nq) or d_hi[0, nq) whatever those
 * arrays hold. */
int sa_locate_device(sa_context* ctx, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lo, const uint32_t* d_hi,
                     uint64_t nq, uint64_t max_hits, uint32_t flags, uint64_t* d_off /* nq + 1 */,
                     uint32_t* d_pos /* may be NULL */, uint64_t pos_cap, uint64_t* total, void* stream);
/* Host in, host out: sa and pos_out have width sa_width (4 or 8).  The host
 * knows the intervals, so it fills off_out and checks before any device work
 * (SA_E_INVALID): an interval with lo > hi or hi > n, pos_cap below the total,
 * a width other than 4 or 8, a width-8 SA entry outside [0, n).  nq == 0 or a
 * total of 0 returns SA_OK without a device. */
int sa_locate(const void* sa, uint64_t n, int sa_width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
              uint64_t max_hits, uint32_t flags, uint64_t* off_out /* nq + 1 */, void* pos_out, uint64_t pos_cap);

/* ---- collections: document array, document frequency and listing ---------
 * (csrc/sa_docs.h).  A collection is a text of n bytes (n <= 2^32 - 1) and
 * D + 1 non-decreasing uint64 offsets doc_off with doc_off[0] = 0 and
 * doc_off[D] = n, 1 <= D <= 2^32 - 2.  Document d is the bytes
 * [doc_off[d], doc_off[d + 1]); empty documents are allowed anywhere and own
 * no position.  The library inserts no separator and reserves no byte; an
 * occurrence belongs to the document in which it STARTS.  A caller who wants
 * no match to span two documents ends each document with a byte the patterns
 * do not contain (it lies inside its document's range).  With the suffix
 * array SA of the text:
 *   doc(p)  = the largest d with doc_off[d] <= p (never an empty document);
 *   DA[r]   = doc(SA[r]);
 *   PRV[r]  = 1 + the largest r' < r with DA[r'] == DA[r], 0 when there is
 *             none: r is the first rank of its document inside [lo, hi)
 *             exactly when PRV[r] <= lo;
 *   df[q]   = #{ r in [lo[q], hi[q]) : PRV[r] <= lo[q] }, the number of
 *             distinct documents of the interval (document frequency);
 *   listing: c[q] = min(df[q], max_docs) (max_docs == 0: no cap), off[0] = 0,
 *             off[q + 1] = off[q] + c[q], and docs[off[q] .. off[q + 1]) = the
 *             DA[r] of the FIRST c[q] qualifying ranks in rank order, then
 *             sorted ascending (sa_locate_device's cap rule: deterministic,
 *             not the max_docs smallest ids).  With SA_DOC_RANK_ORDER the
 *             sort is skipped.
 * The intervals are what sa_find, sa_match, sa_fm_count and sa_repeats give.
 * One that breaks lo <= hi <= n counts as empty, and no load leaves
 * d_prev[0, n), d_da[0, n), d_lo[0, nq) or d_hi[0, nq) whatever those arrays
 * hold.  An interval of up to SA_DOC_GROUP_MAX ranks is counted by a group of
 * 16 lanes; a longer one is cut into chunks of SA_DOC_TILE ranks that
 * workgroups share. */
#define SA_DOC_NONE 0xFFFFFFFFu /* sa_doc_of: the position is not in the text */
#define SA_DOC_RANK_ORDER 1u    /* sa_doc_list: ids in rank order, not sorted */
#define SA_DOC_TILE 2048        /* ranks per chunk of a long interval */
#define SA_DOC_GROUP_MAX 256    /* the longest interval one lane group counts */
#define SA_DOC_LDS_DOCS 8192    /* up to this D the boundaries are searched in LDS, above it in global memory */

/* DA into d_da and PRV into d_prev (n uint32 each, 4-byte aligned; either may
 * be NULL, not both) from d_sa (n uint32) and d_doc_off (D + 1 uint64), all in
 * device memory.  d_sa is not checked: an entry >= n is taken as n - 1.
 * d_doc_off is read at [0, D) only, whatever it holds (the host form checks
 * it in full).  DA alone is one pass and only enqueued on `stream` (no host
 * wait).  PRV sorts the ranks by document with the context's radix sort
 * (sa_sort_pairs_device over the key bits D needs) and scatters neighbours:
 * one host wait, the sort's own, and 24 n bytes of stream-ordered
 * temporaries; the context's workspace grows to n.
 * Checked before any HIP call (SA_E_INVALID): a NULL ctx, d_doc_off or (n > 0)
 * d_sa, both outputs NULL, n too large, D == 0 or D > 2^32 - 2, a misaligned
 * output, an output that is the other output or an input. */
int sa_doc_array_device(sa_context* ctx, uint64_t n, const uint32_t* d_sa, const uint64_t* d_doc_off, uint64_t D,
                        uint32_t* d_da /* may be NULL */, uint32_t* d_prev /* may be NULL */, void* stream);
/* doc(p) into d_doc and p - doc_off[doc(p)] into d_rel (count uint32 each;
 * either may be NULL, not both) for the count positions at d_pos (uint32, what
 * sa_locate_device returns).  A position >= n gives SA_DOC_NONE in both.
 * Asynchronous: no context, no host wait, no temporaries.  The same checks as
 * above without the context. */
int sa_doc_of_device(const uint64_t* d_doc_off, uint64_t D, uint64_t n, const uint32_t* d_pos, uint64_t count,
                     uint32_t* d_doc /* may be NULL */, uint32_t* d_rel /* may be NULL */, void* stream);
/* df[q] (uint32) of nq intervals.  Asynchronous like sa_find_device: no
 * context, no host wait; every d_df[q] is written by the call itself (the
 * chunks of a long interval are added into a word the call has zeroed), so two
 * calls in a row give the same numbers.  The work is the sum of the interval
 * lengths at 4 bytes per rank; one stream-ordered temporary of 8 (nq + 1)
 * bytes.  Checked before any HIP call: NULL pointers (nq > 0), n or nq too
 * large, a misaligned d_df, d_df an input. */
int sa_doc_frequency_device(uint64_t n, const uint32_t* d_prev, const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq,
                            uint32_t* d_df, void* stream);
/* The listing, with sa_locate_device's two-call contract: always fills
 * d_off[0, nq] and *total; ids are written only when d_docs is not NULL and
 * *total <= docs_cap (exactly d_docs[0, total), at any 4-byte alignment);
 * otherwise the call returns SA_OK with *total set and touches nothing in
 * d_docs: the sizing call.  The qualifying ids are materialised (4 bytes each,
 * stream-ordered) and sorted per query by sa_locate_device's kernels, so sorted
 * output needs total <= 2^32 - 1 (SA_E_INVALID otherwise: cap it with
 * max_docs).  A long interval's ids are written by one workgroup.
 * Synchronises `stream`: one host wait for the total; when ids are written,
 * sa_locate_device's own over them (one, more when a query lists more than
 * SA_LOCATE_TILE documents), or one at the end with SA_DOC_RANK_ORDER.
 * Checked before any HIP call: a NULL ctx, total, d_off or (nq > 0) d_da,
 * d_prev, d_lo, d_hi; n or nq too large; unknown flags; a misaligned d_off or
 * d_docs; an output that is an input or the other output. */
int sa_doc_list_device(sa_context* ctx, uint64_t n, const uint32_t* d_da, const uint32_t* d_prev, const uint32_t* d_lo,
                       const uint32_t* d_hi, uint64_t nq, uint64_t max_docs, uint32_t flags, uint64_t* d_off /* nq + 1 */,
                       uint32_t* d_docs /* may be NULL */, uint64_t docs_cap, uint64_t* total, void* stream);
/* Host in, host out, over the staging of the other host forms; they allocate,
 * use and free device buffers.  Arrays of ranks, positions and ids have the
 * given width (4: uint32, 8: int64; SA_DOC_NONE stays 0xFFFFFFFF at width 8);
 * lo, hi, off_out and df_out are uint64.  Checked in full before any device
 * work, each with its own message (SA_E_INVALID): the width; NULL pointers;
 * doc_off not starting at 0, decreasing or not ending at n; D == 0 or too
 * large; an interval with lo > hi or hi > n; docs_cap below the total; a
 * width-8 entry out of range; an output that is an input or another output.
 * sa_doc_list fills off_out on the host from prev, as sa_locate does from the
 * intervals; with docs_out NULL it stops there (the sizing call: the total is
 * off_out[nq]).  n == 0 (sa_doc_array), count == 0, nq == 0 and a total of 0
 * return SA_OK without a device. */
int sa_doc_array(const void* sa, uint64_t n, int sa_width, const uint64_t* doc_off /* D + 1 */, uint64_t D,
                 void* da_out /* may be NULL */, void* prev_out /* may be NULL */);
int sa_doc_of(const uint64_t* doc_off /* D + 1 */, uint64_t D, uint64_t n, const void* pos, uint64_t count, int width,
              void* doc_out /* may be NULL */, void* rel_out /* may be NULL */);
int sa_doc_frequency(const void* prev, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
                     uint64_t* df_out);
int sa_doc_list(const void* da, const void* prev, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi,
                uint64_t nq, uint64_t max_docs, uint32_t flags, uint64_t* off_out /* nq + 1 */, void* docs_out,
                uint64_t docs_cap);

/* ---- longest common extensions: an RMQ index over the LCP array ------------
 * (csrc/sa_lce.h).  LCP as sa_lcp_device writes it: lcp[0] = 0, lcp[r] =
 * lcp(SA[r - 1], SA[r]), n <= 2^32 - 1.  SA_LCE_NONE is the minimum's identity.
 *   lcp_min(lo, hi) of an SA interval [lo, hi) = min lcp[lo + 1 .. hi - 1]: the
 *             length of the longest common prefix of all suffixes of the
 *             interval, its string depth (what find, match, fm_count and
 *             repeats return intervals of).  The empty minimum (hi - lo <= 1)
 *             is SA_LCE_NONE, and so is an interval that breaks lo < hi <= n.
 *   lce(i, j) of two text positions, ISA the inverse suffix array: a position
 *             >= n is the empty suffix and lce = 0 when either is one;
 *             lce(i, i) = n - i; otherwise, with a = min(ISA[i], ISA[j]) and
 *             b = max(ISA[i], ISA[j]), lce(i, j) = min lcp[a + 1 .. b].
 *   order     of the substrings T[i, i + li) and T[j, j + lj), lengths clipped
 *             to the text's end: with l = min(lce(i, j), li, lj), sign(li - lj)
 *             when l == min(li, lj), otherwise -1 when ISA[i] < ISA[j], else
 *             +1; int8 in {-1, 0, +1}.  No text byte is needed.
 * The index is one flat byte buffer of sa_lce_index_bytes(n) bytes that holds
 * offsets and never pointers (16-byte aligned, copyable between devices and
 * to a file): a 4096-byte header (magic, version, n, section offsets), the
 * minima of the blocks of SA_LCE_BLOCK ranks with a sparse table over spans of
 * 1 .. 32 blocks inside each superblock of SA_LCE_SUPER ranks, and a full
 * sparse table over the superblock minima: 4096 + 4 (6 nb + levels ns) bytes
 * rounded up to 16, nb = ceil(n / 64), ns = ceil(nb / 64), levels =
 * floor(log2 ns) + 1 (under 0.40 n + 8 KiB for n >= 2^20).  The build reads
 * LCP once, needs no context and no temporaries and makes no host wait; the
 * header is written last.  n == 0 builds a valid empty index.
 * A query is answered by 16 lanes: two masked blocks of LCP and at most six
 * cells of the tables, all loaded at once (one memory round trip for a rank
 * interval, two for a pair of positions: the ISA gathers first).  With d_text
 * not NULL the position forms first compare SA_LCE_PROBE bytes at i and j and
 * answer from them when the mismatch lies inside; the answers are the same
 * with and without the text.  The kernel checks the header (magic, version,
 * n, every section inside index_bytes): where it does not hold every query
 * answers SA_LCE_NONE (order 0).  Ranks read from d_isa are clamped below n
 * and cells to their section: whatever the arrays hold, no load leaves them.
 * The queries make no host wait and use no temporaries.
 * Rejected before any HIP call, each with its own message (SA_E_INVALID): n or
 * nq above 2^32 - 1; a NULL pointer (d_text may be NULL; d_lcp and d_isa when
 * n == 0); d_index or d_lcp not 16-byte aligned, d_out / d_lce not 4-byte
 * aligned; index_bytes below sa_lce_index_bytes(n) at the build; an output
 * that is an input.  nq == 0 is SA_OK without a launch. */
#define SA_LCE_NONE 0xFFFFFFFFu /* the minimum of no rank */
#define SA_LCE_PROBE 16         /* text bytes compared before ISA, LCP and the index are asked */
#define SA_LCE_BLOCK 64         /* ranks per block */
#define SA_LCE_SUPER 4096       /* ranks per superblock */
/* pure host arithmetic, exact; 0 for n above 2^32 - 1 */
uint64_t sa_lce_index_bytes(uint64_t n);
int sa_lce_build_device(uint64_t n, const uint32_t* d_lcp, void* d_index, uint64_t index_bytes, void* stream);
int sa_lcp_min_device(uint64_t n, const uint32_t* d_lcp, const void* d_index, uint64_t index_bytes,
                      const uint32_t* d_lo, const uint32_t* d_hi, uint64_t nq, uint32_t* d_out, void* stream);
int sa_lce_device(uint64_t n, const uint8_t* d_text /* or NULL */, const uint32_t* d_isa, const uint32_t* d_lcp,
                  const void* d_index, uint64_t index_bytes, const uint32_t* d_i, const uint32_t* d_j, uint64_t nq,
                  uint32_t* d_lce, void* stream);
int sa_substr_compare_device(uint64_t n, const uint8_t* d_text /* or NULL */, const uint32_t* d_isa,
                             const uint32_t* d_lcp, const void* d_index, uint64_t index_bytes, const uint32_t* d_i,
                             const uint32_t* d_li, const uint32_t* d_j, const uint32_t* d_lj, uint64_t nq,
                             int8_t* d_order, void* stream);
/* Host in, host out, over the staging of the other host forms; they allocate,
 * use and free device buffers.  lcp and sa have the given width (4: uint32,
 * 8: int64); lo, hi, i, j, li, lj and the uint32 answers are uint64 (SA_LCE_NONE
 * stays 0xFFFFFFFF), the order int8.  sa_lcp_min builds the index of lcp;
 * sa_lce and sa_substr_compare compute LCP, ISA and the index from (text, sa)
 * (sa must be the suffix array of the text) and probe the text.  A position
 * or length above 2^32 - 1 counts as 2^32 - 1.  Checked before any device
 * work (SA_E_INVALID): the width; n or nq too large; NULL pointers; a width-8
 * entry out of range; an output that is an input.  nq == 0, n == 0 (the
 * position forms) and a batch without any interval of two or more ranks
 * return SA_OK without a device. */
int sa_lcp_min(const void* lcp, uint64_t n, int width, const uint64_t* lo, const uint64_t* hi, uint64_t nq,
               uint64_t* out);
int sa_lce(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint64_t* i, const uint64_t* j,
           uint64_t nq, uint64_t* out);
int sa_substr_compare(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint64_t* i,
                      const uint64_t* li, const uint64_t* j, const uint64_t* lj, uint64_t nq, int8_t* out);

/* ---- k-mismatch pattern search (Hamming distance) --------------------------
 * (csrc/sa_hamming.h).  Text T of n bytes with its suffix array, a batch of nq
 * patterns as sa_find takes them (d_pat, pat_bytes, nq + 1 offsets) and one
 * budget k for the call, 0 <= k <= SA_HAMMING_MAX_K = 255.
 * An occurrence of pattern P of m bytes is a text position p with p + m <= n
 * and d(p) <= k, where d(p) = #{ t : P[t] != T[p + t] }.  Bytes as sa_find has
 * them: binary-safe, 0x00 and 0xFF are ordinary bytes, lengths are explicit.
 * The empty pattern occurs at every p in [0, n) with distance 0 (sa_find's
 * [0, n)); m > n or n == 0 gives no occurrence; m <= k is answered as defined:
 * every p <= n - m is an occurrence (max_candidates is what protects a caller
 * from it).  Budgets per query are not offered.
 * The output is CSR over the queries in sa_locate_device's conventions: off
 * (nq + 1 uint64, off[0] = 0, the total is off[nq]), pos (uint32 text
 * positions, ascending inside each query, every occurrence exactly once) and
 * dist (uint8, d(p) of the same slot; may be NULL when only positions are
 * wanted).
 * info: SA_HAMMING_INFO uint64 on the host: [0] the total (0 with
 * SA_HAMMING_TOO_MANY), [1] the candidates, [2] the pieces searched,
 * nq (k + 1).
 * max_candidates (0 = none) is the only knob: when the seed occurrences exceed
 * it nothing is enumerated and the call returns SA_HAMMING_TOO_MANY (a
 * positive status, as SA_MEM_TOO_MANY) with the info words filled and off all
 * zero.  There is no cap on the hits of a piece: dropping a frequent piece
 * would lose occurrences, and this call is complete or says why not.
 * How it works: piece j = 0 .. k of a pattern is P[b_j, b_{j+1}) with b_j =
 * floor(j m / (k + 1)); an occurrence with d(p) <= k matches at least one of
 * the k + 1 pieces exactly (pigeonhole), so p + b_j is among that piece's
 * exact occurrences.  The pieces of the batch are searched by sa_find_device
 * (an empty piece, m < k + 1, gets [0, n)) and their hits listed by
 * sa_locate_device.  A candidate (pattern, piece j, hit h) with p = h - b_j is
 * kept exactly when it is valid (h >= b_j, p + m <= n), d(p) <= k, and j is
 * the first piece of the pattern that matches T exactly at p: each occurrence
 * passes once, without a sort, a hash or an atomic.  The survivors are
 * compacted and sorted per query by sa_locate_device's sort, whose limit on a
 * sorted total is inherited: more than 2^32 - 1 occurrences in all are
 * SA_E_INVALID.  The distances are computed again for the survivors in output
 * order.  A lane verifies by 8-byte words; the candidates of patterns longer
 * than 8192 bytes go to a wavefront (512 bytes a step).  Temporaries are about
 * 4.2 bytes per candidate on top of sa_locate_device's own, 4 bytes per
 * occurrence and 24 bytes per piece.  DESIGN.md section 21. */
#define SA_HAMMING_MAX_K 255
#define SA_HAMMING_INFO 3
#define SA_HAMMING_TOO_MANY 1
#define SA_HAMMING_LANE 1u   /* tests, A/B: every candidate verified by its own lane */
#define SA_HAMMING_WAVE 2u   /* tests, A/B: every candidate verified by a wavefront */

/* d_text: n bytes, d_sa: n uint32, d_pat: pat_bytes bytes, d_pat_off: nq + 1
 * uint64 (clamped to pat_bytes, a decreasing pair is the empty pattern, as
 * sa_find_device reads them), d_off: nq + 1 uint64, d_pos: out_cap uint32 or
 * NULL, d_dist: out_cap bytes or NULL, all in device memory.  When d_pos is
 * NULL, or when the total exceeds out_cap, d_off and info are filled, nothing
 * in d_pos / d_dist is touched and the call returns SA_OK: the sizing call,
 * after which the caller allocates and calls again.  Exactly [0, total) of
 * d_pos and d_dist and d_off[0, nq] are written; d_pos may have any 4-byte
 * alignment, d_dist any (d_off 8-byte).
 * Synchronises `stream`.  Host waits per call: one for the candidate count,
 * sa_locate_device's own over the pieces (one; two when a piece has more than
 * SA_LOCATE_TILE hits), one for the total, sa_locate_device's own over the
 * survivors (one; more when a query has more than SA_LOCATE_TILE
 * occurrences), and one at the end when d_dist is given.  Temporaries are
 * stream-ordered allocations (SA_E_NOMEM when one fails).
 * nq == 0: SA_OK, off[0] = 0, no kernel.  n == 0: SA_OK, off all zero, no
 * kernel.
 * Checked before any HIP call (SA_E_INVALID, each with its own message): a
 * NULL ctx, info or d_off; a NULL d_text or d_sa with n > 0; a NULL d_pat with
 * pat_bytes > 0; a NULL d_pat_off with nq > 0; n, nq or nq (k + 1) above
 * 2^32 - 1; k above SA_HAMMING_MAX_K; unknown flags (or both of them); d_dist
 * without d_pos; an output that is one of the inputs or another output.
 * Precondition: d_sa is a valid suffix array of the text.  Without it
 * occurrences may be missing, but what is listed is an occurrence with its
 * distance, and no load leaves d_text[0, n), d_sa[0, n), d_pat[0, pat_bytes),
 * the offsets or the temporaries: a hit >= n reads as invalid, the piece
 * offsets are clamped as sa_find_device clamps them, and every compare ends at
 * min(m, n - p). */
int sa_hamming_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                      uint64_t pat_bytes, const uint64_t* d_pat_off /* nq + 1 */, uint64_t nq, uint64_t k,
                      uint64_t max_candidates, uint32_t flags, uint64_t* d_off /* nq + 1 */, uint32_t* d_pos,
                      uint8_t* d_dist, uint64_t out_cap, uint64_t info[SA_HAMMING_INFO], void* stream);
/* Host in, host out over the staging of the other host forms: sa and pos_out
 * have width sa_width (4 or 8; a width-8 SA entry outside [0, n) is
 * SA_E_INVALID before any device work), dist_out is uint8, pat_off must not
 * decrease and pat holds pat_off[nq] bytes.  The total is found first and the
 * device outputs are allocated then, so a caller may pass out_cap = 0 and NULL
 * outputs to learn the total (info[0]) and off_out, and call again.  nq == 0
 * and n == 0 need no device.  Arguments are checked as the device form checks
 * them. */
int sa_hamming(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat,
               const uint64_t* pat_off /* nq + 1 */, uint64_t nq, uint64_t k, uint64_t max_candidates, uint32_t flags,
               uint64_t* off_out /* nq + 1 */, void* pos_out /* width sa_width */, uint8_t* dist_out, uint64_t out_cap,
               uint64_t info[SA_HAMMING_INFO]);

/* ---- k-difference pattern search (edit distance) ---------------------------
 * (csrc/sa_edit.h).  Text T of n bytes with its suffix array, a batch of nq
 * patterns as sa_find takes them and one budget k for the call, 0 <= k <=
 * SA_EDIT_MAX_K = 31 (the band of 2k + 1 <= 63 diagonals fits one 64-bit
 * word).  Substitutions, insertions and deletions cost one each.
 * For an end e in [0, n] let D(e) = min over s <= e of ed(P, T[s, e)), ed the
 * unit-cost Levenshtein distance.  An occurrence of pattern P of m bytes is an
 * end e with D(e) <= k; its distance is D(e) and its start the largest s with
 * ed(P, T[s, e)) = D(e): the shortest best match.  A pattern with m <= k
 * matches at every end: it is not searched and its list is empty, but its
 * pieces are counted in info[2].  A pattern with m > n is searched (T = abc,
 * P = abcd, k = 1: the end 3 at distance 1).  Bytes as sa_find has them.
 * The output is CSR over the queries: off (nq + 1 uint64, off[0] = 0, the
 * total is off[nq]), end (uint32, ascending inside each query, every end
 * exactly once), start (uint32) and dist (uint8) of the same slot; start and
 * dist may each be NULL, and neither may be given without end.
 * info: SA_EDIT_INFO uint64 on the host: [0] the total (0 with
 * SA_EDIT_TOO_MANY), [1] the candidates, [2] the pieces, nq (k + 1).
 * max_candidates (0 = none): when the seed occurrences exceed it nothing is
 * enumerated and the call returns SA_EDIT_TOO_MANY (a positive status, as
 * SA_HAMMING_TOO_MANY) with the info words filled and off all zero.
 * flags: none yet, must be 0.
 * How it works: the pieces are sa_hamming's, b_j = floor(j m / (k + 1)); an
 * alignment with at most k edits leaves one piece untouched, so it passes
 * through an exact occurrence h of piece j, on the diagonal c = h - b_j
 * (signed), and lies within the diagonals c - k .. c + k.  A lane runs the DP
 * over that band for its candidate as a bit-vector kept in registers (a row
 * step is one addition and a dozen logic operations; the row's equality word
 * comes from 8-byte compares of the text against P[i]), stops when the whole
 * row is above k, and leaves a 64-bit mask of the ends it found.  The ends are
 * written in candidate order, sorted per query by sa_locate_device's sort
 * (whose limit is inherited: more than 2^32 - 1 ends before the duplicates are
 * removed are SA_E_INVALID), and the first of each run is kept.  Distances and
 * starts come from the DP anchored at the end and run backwards over the
 * diagonals -k .. k, once per end; it is skipped when neither is asked for.
 * Temporaries are about 12.2 bytes per candidate on top of sa_locate_device's
 * own, 8 bytes and a sort per end found and 24 bytes per piece.  DESIGN.md
 * section 23. */
#define SA_EDIT_MAX_K 31
#define SA_EDIT_INFO 3
#define SA_EDIT_TOO_MANY 1

/* The buffers are sa_hamming_device's, with d_end / d_start (out_cap uint32
 * each, any 4-byte alignment) and d_dist (out_cap bytes) in place of d_pos /
 * d_dist.  When d_end is NULL, or when the total exceeds out_cap, d_off and
 * info are filled, nothing in d_end / d_start / d_dist is touched and the call
 * returns SA_OK: the sizing call, after which the caller allocates and calls
 * again.  The sizing call does all the work but the backward DP.  Exactly
 * [0, total) of the outputs given and d_off[0, nq] are written.
 * Synchronises `stream`.  Host waits per call: one for the candidate count,
 * sa_locate_device's own over the pieces, one for the ends found,
 * sa_locate_device's own over them, one for the total and one at the end.
 * nq == 0: SA_OK, off[0] = 0, no kernel.  n == 0: SA_OK, off all zero, no
 * kernel.
 * Checked before any HIP call (SA_E_INVALID, each with its own message, and
 * nothing is written): a NULL ctx, info or d_off; a NULL d_text or d_sa with
 * n > 0; a NULL d_pat with pat_bytes > 0; a NULL d_pat_off with nq > 0; n, nq
 * or nq (k + 1) above 2^32 - 1; k above SA_EDIT_MAX_K; flags other than 0;
 * d_start or d_dist without d_end; an output that is one of the inputs or
 * another output.
 * Precondition: d_sa is a valid suffix array of the text.  Without it
 * occurrences may be missing, but no load leaves d_text[0, n), d_sa[0, n),
 * d_pat[0, pat_bytes), the offsets or the temporaries: a hit >= n reads as no
 * candidate and every text window is clipped to [0, n). */
int sa_edit_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                   uint64_t pat_bytes, const uint64_t* d_pat_off /* nq + 1 */, uint64_t nq, uint64_t k,
                   uint64_t max_candidates, uint32_t flags, uint64_t* d_off /* nq + 1 */, uint32_t* d_end,
                   uint32_t* d_start, uint8_t* d_dist, uint64_t out_cap, uint64_t info[SA_EDIT_INFO], void* stream);
/* Host in, host out as sa_hamming: sa, end_out and start_out have width
 * sa_width (4 or 8), dist_out is uint8, pat_off must not decrease.  The total
 * is found first and the device outputs are allocated then, so a caller may
 * pass out_cap = 0 and NULL outputs to learn the total (info[0]) and off_out,
 * and call again.  nq == 0 and n == 0 need no device.  Arguments are checked
 * as the device form checks them. */
int sa_edit(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat,
            const uint64_t* pat_off /* nq + 1 */, uint64_t nq, uint64_t k, uint64_t max_candidates, uint32_t flags,
            uint64_t* off_out /* nq + 1 */, void* end_out /* width sa_width */, void* start_out /* width sa_width */,
            uint8_t* dist_out, uint64_t out_cap, uint64_t info[SA_EDIT_INFO]);

/* ---- maximal exact matches of a query against the text -------------------
 * (csrc/sa_mem.h).  Text T of n bytes with its suffix array, query Q of m
 * bytes, min_len = L >= 1.  A MEM is a triple (i, p, l) with all of:
 *   Q[i .. i + l) == T[p .. p + l) and l >= L;
 *   no extension to the right: i + l == m, or p + l == n, or Q[i + l] != T[p + l];
 *   no extension to the left:  i == 0, or p == 0, or Q[i - 1] != T[p - 1].
 * Bytes as sa_find has them: binary-safe, 0x00 and 0xFF are ordinary bytes.
 * The output is every MEM exactly once, ordered by (i, p) ascending, in CSR
 * form over the query positions: off (m + 1 uint64, off[0] = 0; the MEMs that
 * start at query position i are entries off[i] .. off[i + 1)), tpos (uint32
 * text positions) and len (uint32 lengths; l <= min(n, m)).  The total is
 * off[m].
 * max_occ (0 = none): a query position whose seed Q[i .. i + L) occurs more
 * than max_occ times in the text contributes no MEM and is counted as
 * skipped; that is, a MEM is dropped exactly when its first L bytes occur more
 * than max_occ times.  This is the one knob that bounds the work: the work is
 * proportional to the candidates, the sum of the seed occurrences over the
 * positions that are not skipped.
 * max_candidates (0 = none): when the candidates exceed it nothing is
 * enumerated and the call returns SA_MEM_TOO_MANY (a positive status, as
 * sa_check's) with the info words filled and off all zero.  Temporaries are
 * about 4 bytes per candidate on top of sa_locate_device's own for that many
 * hits, plus 20 bytes per query position.
 * info: SA_MEM_INFO uint64 on the host: [0] the total (0 with
 * SA_MEM_TOO_MANY), [1] the candidates, [2] the skipped positions.
 * How it works: seeds by sa_matching_stats_device with max_len = L, their
 * hits by sa_locate_device (so the candidates are in (i, p) order), then the
 * MEM list is a stable compaction of the candidate list: a candidate stays
 * iff it is left-maximal, and each one that stays is extended to the right.
 * A lane extends by 8-byte words; in auto mode it hands an extension that
 * passes 512 bytes to a wavefront (512 bytes a step).  DESIGN.md section 14. */
#define SA_MEM_INFO 3
#define SA_MEM_TOO_MANY 1
#define SA_MEM_LANE 1u   /* tests, A/B: every right extension by its own lane */
#define SA_MEM_WAVE 2u   /* tests, A/B: every right extension by a wavefront */

/* d_text: n bytes, d_sa: n uint32, d_query: m bytes, d_off: m + 1 uint64,
 * d_tpos / d_len: out_cap uint32 each or both NULL, all in device memory; n
 * and m <= 2^32 - 1.  d_tpos and d_len are both given or both NULL (one of
 * them NULL is SA_E_INVALID).  When they are NULL, or when the total exceeds
 * out_cap, d_off and info are filled, nothing in d_tpos / d_len is touched
 * and the call returns SA_OK: the sizing call, after which the caller
 * allocates and calls again.  Exactly [0, total) of d_tpos and d_len and
 * d_off[0, m] are written; the outputs may have any 4-byte alignment (d_off
 * 8-byte).
 * Synchronises `stream`.  Host waits per call: one for the seed counts,
 * sa_locate_device's own (one; more when a position has more than
 * SA_LOCATE_TILE hits), and one for the total.  Temporaries are
 * stream-ordered allocations (SA_E_NOMEM when one fails).
 * n == 0, m == 0 or L > min(n, m): SA_OK, total 0, off all zero, info zero,
 * no kernel.  L == 0 is SA_E_INVALID.
 * Checked before any HIP call (SA_E_INVALID, each with its own message): a
 * NULL ctx; a NULL d_text or d_sa with n > 0; a NULL d_query with m > 0; a
 * NULL d_off or info; n or m above 2^32 - 1; unknown flags (or both of them);
 * an output that is one of the inputs or another output.
 * Precondition: d_sa is a valid suffix array of the text.  Without it the
 * results are unspecified, but no load leaves the four input buffers: an SA
 * entry >= n is clamped to n - 1, p - 1 and p + l never index outside [0, n),
 * and every extension loop ends at min(n - p, m - i). */
int sa_mems_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query,
                   uint64_t m, uint64_t min_len, uint64_t max_occ, uint64_t max_candidates, uint32_t flags,
                   uint64_t* d_off /* m + 1 */, uint32_t* d_tpos, uint32_t* d_len, uint64_t out_cap,
                   uint64_t info[SA_MEM_INFO], void* stream);
/* Host in, host out: sa, tpos_out and len_out have width sa_width (4 or 8; a
 * width-8 SA entry outside [0, n) is SA_E_INVALID before any device work).
 * The total is found first and the device outputs are allocated then, so a
 * caller may pass out_cap = 0 and NULL outputs to learn the total (info[0])
 * and off_out, and call again.  The three returns without a kernel above need
 * no device.  Arguments are checked as the device form checks them. */
int sa_mems(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* query, uint64_t m,
            uint64_t min_len, uint64_t max_occ, uint64_t max_candidates, uint32_t flags,
            uint64_t* off_out /* m + 1 */, void* tpos_out, void* len_out /* width sa_width */, uint64_t out_cap,
            uint64_t info[SA_MEM_INFO]);

/* ---- longest previous factor and LZ77 factorisation ----------------------
 * (csrc/sa_lz.h).  Text T of n bytes (n <= 2^32 - 1), its suffix array SA and
 * LCP as sa_lcp_device defines it (lcp[0] = 0, lcp[r] = lcp(SA[r - 1],
 * SA[r])).  Bytes are binary-safe; the end of the string sorts smallest.
 * LPF[i] = max { l : some j < i has T[j .. j + l) == T[i .. i + l) }; the
 * earlier occurrence may overlap position i; LPF[0] = 0.
 * SRC[i], canonical (so two calls agree bit for bit): with r the rank of
 * suffix i, a the largest rank < r with SA[a] < i and b the smallest rank > r
 * with SA[b] < i (either may be absent), la = min lcp(a + 1 .. r] and lb =
 * min lcp(r + 1 .. b] (0 for an absent side): LPF[i] = max(la, lb); SRC[i] =
 * SA[a] when la >= lb and la > 0, else SA[b] when lb > 0, else SA_LPF_NONE,
 * which can never be a position.
 * LZ77, greedy and self-referential: phrase starts p0 = 0, p(k+1) = p(k) +
 * max(1, LPF[p(k)]) until n is reached; phrase k is (pos = p(k), len = max(1,
 * LPF[p(k)]), src = SRC[p(k)]).  A literal has len 1 and src SA_LPF_NONE; its
 * byte is T[pos].  z is the number of phrases, emitted in text order.
 * The cost does not depend on the lengths: they are LCP range minima gathered
 * during the nearest-smaller search, the text is never compared.  DESIGN.md
 * section 15. */
#define SA_LPF_NONE 0xFFFFFFFFu

/* d_sa, d_lcp: n uint32; d_lpf, d_src: n uint32 each, in text order, at any
 * 4-byte alignment (they are written by 4-byte scatters); all in device
 * memory.  With d_lcp given the text is not read and d_text may be NULL; with
 * d_lcp == NULL the LCP array is computed by sa_lcp_device's path into a
 * stream-ordered temporary (d_text: n bytes).
 * Enqueued on `stream`.  Host waits per call: none with d_lcp given (the call
 * does not wait for the stream); sa_lcp_device's own without.  Temporaries
 * are stream-ordered allocations (n / 8 bytes, plus 4 n for the LCP array;
 * SA_E_NOMEM when one fails).
 * n == 0: SA_OK, no kernel.  n == 1: LPF = [0], SRC = [SA_LPF_NONE].
 * Checked before any HIP call (SA_E_INVALID, each with its own message): a
 * NULL ctx; n above 2^32 - 1; with n > 0 a NULL d_sa, d_lpf or d_src, d_text
 * and d_lcp both NULL, an output that is not 4-byte aligned, an output that
 * is one of the inputs or the other output.
 * Precondition: d_sa is the text's suffix array and d_lcp its LCP array.
 * Without it the results are unspecified, but no load or store leaves the
 * buffers: an SA entry >= n is clamped to n - 1 and every walk ends at rank 0
 * or n - 1. */
int sa_lpf_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                  const uint32_t* d_lcp /* may be NULL */, uint32_t* d_lpf, uint32_t* d_src, void* stream);
/* The parse.  d_lpf, d_src: n uint32 as sa_lpf_device writes them; d_pos,
 * d_len, d_fsrc: out_cap uint32 each at any 4-byte alignment, all three given
 * or all three NULL.  Neither the text nor the SA is needed.  With NULL
 * outputs, or when z exceeds out_cap, only *z is filled and nothing else is
 * touched: the sizing call, after which the caller allocates and calls again.
 * Exactly [0, z) of each output is written.
 * Synchronises `stream`.  Host waits per call: three (the candidate count,
 * the candidate list, z).  Temporaries are stream-ordered allocations (about
 * 5.2 n bytes; SA_E_NOMEM when one fails).
 * n == 0: SA_OK, z = 0, no kernel.
 * next(i) = i + max(1, LPF[i]) is computed in 64 bits and clamped to n, so an
 * arbitrary d_lpf terminates and stays inside the buffers; its results are
 * unspecified.
 * Checked before any HIP call (SA_E_INVALID, each with its own message): a
 * NULL ctx or z; n above 2^32 - 1; outputs of which only some are NULL; with
 * n > 0 a NULL d_lpf or d_src, an output that is not 4-byte aligned, an output
 * that is one of the inputs or another output. */
int sa_lz77_device(sa_context* ctx, uint64_t n, const uint32_t* d_lpf, const uint32_t* d_src, uint32_t* d_pos,
                   uint32_t* d_len, uint32_t* d_fsrc, uint64_t out_cap, uint64_t* z, void* stream);
/* Host in, host out: sa and the outputs have width sa_width (4 or 8; a
 * width-8 SA entry outside [0, n) is SA_E_INVALID before any device work, and
 * an SA that is not the text's is SA_E_INVALID).  "None" is all ones at
 * either width (-1 as int64).  sa_lz77 computes LPF on the device once, finds
 * z, and writes the phrases when the outputs are given and z <= out_cap; so
 * out_cap = 0 with NULL outputs is the sizing call.  n == 0 needs no device. */
int sa_lpf(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* lpf_out, void* src_out);
int sa_lz77(const uint8_t* text, uint64_t n, const void* sa, int sa_width, void* pos_out, void* len_out, void* src_out,
            uint64_t out_cap, uint64_t* z);

/* ---- repeats: right-maximal, maximal and supermaximal ---------------------
 * (csrc/sa_repeats.h).  Text T of n bytes (n <= 2^32 - 1), its suffix array SA
 * and LCP as sa_lcp_device defines it (lcp[0] = 0, lcp[r] = lcp(SA[r - 1],
 * SA[r])); lcp[n] reads as 0.  Intervals are half-open.
 * A repeat is (len, lo, hi) with len >= 1 and hi - lo >= 2: lcp[lo] < len,
 * lcp[k] >= len for lo < k < hi with equality for some k, lcp[hi] < len.  Its
 * string T[SA[lo] .. SA[lo] + len) occurs exactly at SA[lo .. hi) and is
 * right-maximal: its occurrences are not all followed by the same byte (the
 * end of the text is a follower of its own).  These are the LCP intervals,
 * the internal nodes of the suffix tree other than the root.  The head of a
 * repeat is the smallest k in (lo, hi) with lcp[k] == len; a rank is the head
 * of at most one repeat.  prev(k) = T[SA[k] - 1], and a 257th symbol that
 * differs from every byte when SA[k] == 0.
 *   SA_REP_RIGHT         every repeat.
 *   SA_REP_MAXIMAL       those that are left-maximal too: prev(k), lo <= k <
 *                        hi, are not all equal.
 *   SA_REP_SUPERMAXIMAL  lcp[k] == len for all lo < k < hi and the prev(k),
 *                        lo <= k < hi, are pairwise distinct (so hi - lo <=
 *                        257): a maximal repeat that is no proper substring
 *                        of another maximal repeat.
 * Filters: len >= min_len (0 reads as 1) and hi - lo >= min_occ (0 and 1 read
 * as 2).  Order: ascending head, so two calls agree bit for bit.
 * info[0] = the number of repeats listed, info[1] = the sum of hi - lo over
 * them (the pos_cap of sa_locate_device for all their occurrences: d_lo and
 * d_hi are what it takes).  DESIGN.md section 16. */
#define SA_REP_RIGHT 0
#define SA_REP_MAXIMAL 1
#define SA_REP_SUPERMAXIMAL 2
#define SA_REP_INFO 2

/* d_sa, d_lcp: n uint32; d_len, d_lo, d_hi: out_cap uint32 each at any 4-byte
 * alignment, all three given or all three NULL; all in device memory.  With
 * NULL outputs, or when info[0] exceeds out_cap, only info is filled and
 * nothing else is touched: the sizing call, after which the caller allocates
 * and calls again.  Otherwise exactly [0, info[0]) of each output is written.
 * SA_REP_RIGHT with d_lcp given reads neither the text nor the SA: d_text and
 * d_sa may be NULL.  With d_lcp == NULL the LCP array is computed by
 * sa_lcp_device's path into a stream-ordered temporary.
 * Synchronises `stream`.  Host waits per call: one with d_lcp given (info,
 * after everything is enqueued; the writing kernel reads the count on the
 * device); sa_lcp_device's own and that one without.  Temporaries are
 * stream-ordered allocations (about 0.38 n bytes for SA_REP_MAXIMAL, 0.19 n
 * for the other kinds, plus 4 n for the LCP array; SA_E_NOMEM when one fails).
 * n <= 1: SA_OK, info = {0, 0}, no kernel.
 * Checked before any HIP call (SA_E_INVALID, each with its own message): a
 * NULL ctx or info; n above 2^32 - 1; an unknown kind; outputs of which only
 * some are NULL; with n > 1 a NULL d_text or d_sa where the kind or a NULL
 * d_lcp needs it, an output that is not 4-byte aligned, an output that is one
 * of the inputs or another output.
 * Precondition: d_sa is the text's suffix array and d_lcp its LCP array.
 * With an arbitrary d_sa or d_lcp given the results are unspecified, but no
 * load or store leaves the buffers and info[0] <= out_cap holds for what is
 * written: an SA entry >= n is clamped for the text gather, every walk ends
 * at rank 0 or n, the supermaximal scan stops after 257 ranks. */
int sa_repeats_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                      const uint32_t* d_lcp /* may be NULL */, uint64_t min_len, uint64_t min_occ, uint32_t kind,
                      uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi, uint64_t out_cap, uint64_t info[SA_REP_INFO],
                      void* stream);
/* Host in, host out: sa and the outputs have width sa_width (4 or 8; a
 * width-8 SA entry outside [0, n) is SA_E_INVALID before any device work, and
 * an SA that is not the text's is SA_E_INVALID: it is checked against the text
 * first).  One device computation: the repeats are written into device
 * buffers of min(out_cap, n) entries and copied out when the outputs are
 * given and info[0] <= out_cap; out_cap = 0 with NULL outputs is the sizing
 * call.  n <= 1 needs no device. */
int sa_repeats(const uint8_t* text, uint64_t n, const void* sa, int sa_width, uint64_t min_len, uint64_t min_occ,
               uint32_t kind, void* len_out, void* lo_out, void* hi_out /* width sa_width */, uint64_t out_cap,
               uint64_t info[SA_REP_INFO]);

/* ---- building blocks of the range-partitioned multi-GPU build ----------
 * (hpc_suffix_array_amd/distributed.py drives these per rank; the exchange
 * steps between them are RCCL collectives over xGMI.)                      */

/* 256-bit byte-presence mask of the n device bytes (host out: 8 words). */
int sa_alphabet_device(const uint8_t* d_text, uint64_t n, uint32_t present_out[8], void* stream);

/* Packed K-symbol keys of positions [lo, hi) of the n-byte text:
 * key(i) = sum_t code[text[i+t]] * base^(K-1-t) (0 past the end);
 * code = 256 dense symbol codes (host array), base^K <= 2^64. */
int sa_pack_keys_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, uint64_t lo, uint64_t hi,
                        const uint16_t code[256], uint64_t base, uint32_t K, uint64_t* d_keys_out,
                        void* stream);

/* Stable LSD radix sort of m (u64 key, u32 value) pairs by key bits
 * [0, bits) into keys_out / vals_out (may not alias the inputs). */
int sa_sort_pairs_device(sa_context* ctx, const uint64_t* d_keys_in, const uint32_t* d_vals_in, uint64_t m,
                         uint32_t bits, uint64_t* d_keys_out, uint32_t* d_vals_out, void* stream);

/* dst[idx[i] - base] = src[i] for i < m (8-byte values, int64 indices):
 * the owner-side scatters of the exchange steps (new ranks, SA slices).
 * Indices outside [base, base + dst_n) are skipped and reported as
 * SA_E_INVALID; synchronous on `stream`. */
int sa_scatter_u64_device(uint64_t* d_dst, uint64_t dst_n, const int64_t* d_idx, int64_t base,
                          const uint64_t* d_src, uint64_t m, void* stream);

/* dst[i] = src[idx[i] - base] for i < m (8-byte values, int64 indices):
 * the permutations of the exchange steps.  Indices outside
 * [base, base + src_n) read 0 and are reported as SA_E_INVALID. */
int sa_gather_u64_device(uint64_t* d_dst, const uint64_t* d_src, uint64_t src_n, const int64_t* d_idx, int64_t base,
                         uint64_t m, void* stream);

/* In-place inclusive running max of m int64 values (the group-start
 * carries of the distributed re-rank); asynchronous on `stream`. */
int sa_running_max_i64_device(int64_t* d_v, uint64_t m, void* stream);
/* In-place inclusive prefix sum of m int64 values; asynchronous. */
int sa_inclusive_sum_i64_device(int64_t* d_v, uint64_t m, void* stream);
/* d_out[i] = the number of d_sorted[0 .. m) (non-decreasing) below d_q[i]
 * (at most d_q[i] when right != 0), for i < nq; asynchronous. */
int sa_count_below_u64_device(const uint64_t* d_sorted, uint64_t m, const uint64_t* d_q, uint64_t nq, int right,
                              int64_t* d_out, void* stream);
/* Positions (int64, in order) of the non-zero bytes of d_mask[0 .. m) into
 * d_out (capacity m; NULL: count only); *count = their number.
 * Synchronises `stream`. */
int sa_select_u8_device(const uint8_t* d_mask, uint64_t m, int64_t* d_out, uint64_t* count, void* stream);

/* ---- range-partitioned multi-GPU build, per rank ------------------------
 * Replaces src/mpi/manber_myers_mpi.c:22-160 (and main_mpi.c:43-54).  Every
 * rank holds the whole text in HBM; the SA is split into `world` contiguous
 * ranges of buckets (the first symbols of a suffix), rank q sorting the
 * suffixes of its range, which land at SA positions [sa_off, sa_off + m).
 * Sequence per build (the caller runs the collectives in brackets; see
 * hpc_suffix_array_amd/distributed.py):
 *   [all_reduce MAX of the 256-bit alphabet masks of the ranks' slices]
 *   sa_dist_begin   -> coarse bucket histogram of this rank's slice (d_coarse)
 *   [all_reduce SUM of d_coarse, copied to the host]
 *   sa_dist_cuts    -> m, sa_off (identical cuts on every rank)
 *   sa_dist_round1  -> the first round of the range into d_sa_local (m uint32)
 *   per round h = K, 2K, ... while any rank has unsorted suffixes:
 *     sa_dist_req_count -> requests per owner   [all_gather of counts]
 *     sa_dist_req_fill  -> requests by owner     [all_to_all]
 *     sa_dist_answer    -> ranks of the received requests   [all_to_all back]
 *     sa_dist_refine    -> sort / re-rank the unsorted set
 * status: SA_DIST_OK, or a reason the caller must build another way (all
 * ranks agree on it through a collective). */
#define SA_DIST_OK 0
#define SA_DIST_UNSUPPORTED 1   /* one symbol, or no bucketed key layout for this n */
#define SA_DIST_UNBALANCED 2    /* the bucket ranges cannot balance (skewed text) */

typedef struct {
    int32_t status;         /* SA_DIST_* */
    int32_t sigma;          /* distinct symbols */
    int32_t K;              /* symbols sorted by the first round */
    int32_t bucket_bits;    /* bucket = first symbols, bucket_bits wide */
    uint64_t m;             /* suffixes of this rank's range */
    uint64_t sa_off;        /* its first SA position */
    uint64_t m_max;         /* largest range over all ranks */
    uint32_t bucket_lo, bucket_hi;   /* this rank's buckets [lo, hi) */
    int32_t round1_ok;      /* 0: a window exceeded the LDS tile (fall back) */
    int32_t reserved;
    uint64_t heads;         /* groups completed in the last phase (local) */
    uint64_t unsorted;      /* this rank's unsorted suffixes after it */
    uint64_t groups;        /* their groups */
} sa_dist_info;

/* present: OR of all ranks' alphabet masks; d_coarse: 4096 uint64 (world > 1) */
int sa_dist_begin(sa_context* ctx, const uint8_t* d_text, uint64_t n, int world, int rank,
                  const uint32_t present[8], uint64_t* d_coarse, void* stream, sa_dist_info* info);
/* h_coarse: the all-reduced coarse histogram on the host (NULL at world 1) */
int sa_dist_cuts(sa_context* ctx, const uint64_t* h_coarse, sa_dist_info* info);
/* Allocate ahead of the first build everything a range build of up to
 * max_n symbols over `world` ranks needs (sa_dist_cuts would otherwise do it
 * inside the first build). */
int sa_dist_reserve(sa_context* ctx, uint64_t max_n, int world);
/* Frees the range-partitioned build's per-rank buffers of ctx (rank and
 * member arrays, request buffers); the context stays usable (a fallback
 * driver reuses its workspace).  Synchronises the device first. */
int sa_dist_release(sa_context* ctx);
/* The cut plan sa_dist_cuts applies (host only, no device): world + 1 cuts
 * into the 4096 coarse buckets of h_coarse (summing to n) at bucket width
 * bucket_bits; every range holds at most 2^18 buckets.  Returns SA_DIST_OK or
 * SA_DIST_UNBALANCED (largest range m_max above 1.5x the mean), < 0 on bad
 * arguments. */
int sa_dist_plan_cuts(int world, uint64_t n, int bucket_bits, const uint64_t* h_coarse, uint32_t* cuts_out,
                      uint64_t* m_max);
/* d_sa_local: info->m uint32 (global text positions, SA order) */
int sa_dist_round1(sa_context* ctx, uint32_t* d_sa_local, void* stream, sa_dist_info* info, sa_stats* stats);
/* counts_out: world uint64 -- requests this rank sends to each rank */
int sa_dist_req_count(sa_context* ctx, uint64_t h, uint64_t* counts_out, void* stream, sa_dist_info* info);
/* d_req: sum(counts_out) uint32, grouped by destination rank */
int sa_dist_req_fill(sa_context* ctx, uint64_t h, uint32_t* d_req, void* stream);
/* ranks of nreq received positions (all in this rank's range) -> d_ans (uint64) */
int sa_dist_answer(sa_context* ctx, const uint32_t* d_req, uint64_t nreq, uint64_t* d_ans, void* stream);
/* d_ans: the answers to this rank's requests, in request order */
int sa_dist_refine(sa_context* ctx, uint64_t h, const uint64_t* d_ans, uint32_t* d_sa_local, void* stream,
                   sa_dist_info* info);

/* Seeded synthetic text in device memory: the splitmix64 generator of
 * SURVEY.md 8(d) (symbol i = alphabet[((z >> 32) * sigma) >> 32]); the
 * stand-in for scripts/generate_large_datasets.py:12-28, seeded. */
int sa_generate_text_device(uint8_t* d_out, uint64_t n, uint64_t seed, const uint8_t* alphabet,
                            uint32_t sigma, void* stream);

const char* sa_last_error(void);
/* number of visible HIP devices (0 when none; never aborts) */
int sa_device_count(void);
/* library build identification, e.g. "sa_hip gfx950 <date>" */
const char* sa_version(void);
/* Host waits (stream synchronisations and blocking copies) the library has
 * made in this process so far; a driver differences it around a build. */
uint64_t sa_host_syncs(void);

/* sizeof(sa_stats) (which = 0) / sizeof(sa_opts) (which = 1), for bindings */
uint64_t sa_struct_size(int which);

#ifdef __cplusplus
}
#endif

#endif /* SA_HIP_H */
