// sa_packed.h -- the packed schedule: round 1 sorts every suffix by its first
// K symbols, doubling rounds then run over the unsorted set only (build_packed:
// plan_round1, round1, doubling_rounds).  Included by sa_build.hip in namespace sa.
#pragma once

// K for base B: largest K with B^K - 1 < 2^64
static uint32_t max_chars(uint64_t base) {
    uint32_t K = 0;
    uint64_t prod = 1;
    while (prod <= UINT64_MAX / base) {
        prod *= base;
        ++K;
    }
    return K;
}

static uint32_t key_bits(uint64_t base, uint32_t K) {   // bit width of B^K - 1
    unsigned __int128 p = 1;
    for (uint32_t t = 0; t < K; ++t) p *= base;
    p -= 1;
    uint32_t w = 0;
    while (p) { ++w; p >>= 1; }
    return w;
}

// the fewest symbols K with sigma^K >= 512 n: a random text of this
// alphabet then leaves few suffixes unsorted by round 1
static uint32_t min_chars(uint32_t sigma, uint64_t n) {
    const uint32_t kmax = max_chars((uint64_t)sigma + 1);
    uint32_t kmin = 1;
    unsigned __int128 p = sigma, target = (unsigned __int128)n * 512u;
    while (p < target && kmin < kmax) {
        p *= sigma;
        ++kmin;
    }
    return kmin;
}

// auto K: min_chars, rounded up to fill the radix passes (the LSD round 1).
static uint32_t choose_chars(uint32_t sigma, uint64_t n, int32_t req) {
    const uint64_t base = (uint64_t)sigma + 1;
    const uint32_t kmax = max_chars(base);
    if (req > 0) return std::min<uint32_t>((uint32_t)req, kmax);
    if (sigma <= 1) return kmax;
    const uint32_t kmin = min_chars(sigma, n);
    const uint32_t P = (key_bits(base, kmin) + 7) / 8;
    uint32_t K = kmin;
    while (K + 1 <= kmax && key_bits(base, K + 1) <= 8 * P) ++K;
    return K;
}

// segments(): ranks, SA positions and the next unsorted set from sorted pairs
struct SegSrc {
    const uint64_t* keys;
    const uint32_t* idx;
    Chunking ch;
};
// Where the ranks and the next set go when not to the context's rank array and
// the start of set uo.  rank_arr / rank_off / rm: the range-partitioned build's
// compact rank map and its SA offset (sa_dist.h).  set_off / g_off: the set's
// first slot and group id (after a pivot round's tied blocks).  gsn: the set's
// group starts are written here too (or null).
struct SegDest {
    uint32_t* rank_arr = nullptr;
    uint64_t rank_off = 0;
    RankMap rm = RankMap{};
    uint64_t set_off = 0;
    uint32_t g_off = 0;
    uint32_t* gsn = nullptr;
};
struct SegResult {
    SetTotals t;
    bool sparse = false;   // ranks were kept for the unsorted suffixes only (member bitmap)
};

template <class Pos>
static int segments(Run& r, const SegSrc& src, Pos pos, bool sparse_ok, uint32_t* sa, int uo, SegResult* out,
                    const SegDest& d = SegDest{}) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    const Chunking& ch = src.ch;
    uint32_t* const rank_arr = d.rank_arr ? d.rank_arr : c->rank;
    uint32_t* c_h = c->counts;
    uint32_t* c_u = c->counts + kMaxChunks;
    uint32_t* c_uh = c->counts + 2 * kMaxChunks;
    uint32_t* c_l = c->counts + 3 * kMaxChunks;
    r.begin(SA_K_SEG_COUNT);
    hipLaunchKernelGGL(k_seg_count, dim3(ch.chunks), dim3(kBlock), 0, s, src.keys, ch, c_h, c_u, c_uh, c_l);
    r.end();
    r.begin(SA_K_SEG_SCAN);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(kBlock), 0, s, c_h, c_u, c_uh, c_l, ch.chunks, c->words);
    r.end();
    SA_HIP(hipGetLastError());
    SA_READ(hwd, read_words(c, 20, s));
    if (hwd[kLookbackWord]) return set_err(SA_E_INTERNAL, "radix look-back did not complete");
    out->t = totals_of(hwd);
    // first round with few unsorted suffixes: keep ranks only for those
    const bool sparse = sparse_ok && out->t.m <= ch.n / kSparseDiv;
    out->sparse = sparse;
    if (sparse) SA_HIP(hipMemsetAsync(c->member, 0, (ch.n + 31) / 32 * 4, s));
    r.begin(SA_K_SEG_WRITE);
    hipLaunchKernelGGL(k_seg_write<Pos>, dim3(ch.chunks), dim3(kBlock), 0, s, src.keys, src.idx, ch, pos,
                       (const uint32_t*)c_u, (const uint32_t*)c_uh, (const uint32_t*)c_l, rank_arr, sa,
                       c->u_pos[uo] + d.set_off, c->u_idx[uo] + d.set_off, c->u_g[uo] + d.set_off,
                       sparse ? c->member : nullptr, sparse ? 0 : 1, (uint32_t)d.rank_off, d.rm, d.g_off, d.gsn ? d.gsn + d.g_off : nullptr,
                       (uint32_t)d.set_off);
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_SEG_COUNT, 8 * ch.n);
    r.bytes(SA_K_SEG_SCAN, 32ull * ch.chunks);
    r.bytes(SA_K_SEG_WRITE, ch.n * (8 + (sparse ? 0 : 8)) + (sa ? 8 * ch.n : 0) + out->t.m * 16);
    return SA_OK;
}

// Sorting an unsorted set by (group, rank[x + h]), shared with sa_dist.h.  The
// per-group register sort is tried when the average group holds at most kUsAvg
// suffixes, under the flag protocol: kUsFlagWord zeroed, the caller's launches
// (which raise it on a group over kUsLimit), the flag read back.  *sorted: no
// group was too large, the launches' output stands.
constexpr uint64_t kUsAvg = 4;
template <class Launch>
static int usort_try(Run& r, Launch launch, bool* sorted) {
    SA_HIP(hipMemsetAsync(r.c->words + kUsFlagWord, 0, 4, r.s));
    r.begin(SA_K_SORT_U);
    launch();
    r.end();
    SA_HIP(hipGetLastError());
    SA_READ(flag, read_word(r.c, kUsFlagWord, r.s));
    *sorted = *flag == 0;
    return SA_OK;
}

// Else the radix sort: the `bits`-bit keys written once into b.kb1 with the digit
// totals (the first pass reads them there, the second overwrites them), then
// sorted.  before(): the caller's launches after the totals' reset (key1 samples).
template <class Src, class Before>
static int usort_radix(Run& r, const Src& src, const uint32_t* u_idx, uint64_t m, uint32_t bits, const SortBufs& b,
                       Before before, Sorted* out) {
    sa_context* const c = r.c;
    SA_TRY(onesweep_prepare(c, r.s));
    const uint32_t Pu = (bits + 7) / 8;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((m + kBlock - 1) / kBlock, 2048);
    SA_TRY(before());
    r.begin(SA_K_SORT_U);
    hipLaunchKernelGGL(k_materialize<Src>, dim3(grid), dim3(kBlock), 0, r.s, src, m, Pu, b.kb1, os_ghist(c));
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_SORT_U, 16 * m);
    return radix_sort(r, SrcKeys{b.kb1, u_idx}, 12 * m, plan_chunks(m), bits, b, out, SortFlags{true, true});
}

// Unsorted-set round by a three-way pivot split: dense ranks, large groups
// on average.
static bool pivot_ok(const sa_context* c, uint64_t m, uint64_t G, uint32_t wr, bool sparse) {
    return !(c->dbg & SA_DEBUG_NO_PIVOT) && c->radix == 0 && !sparse && m >= (1u << 16) && G >= 1 && G <= m / 4 && bit_width(2 * G + 1) + wr <= 64;
}

// tied-block rounds scan the groups in one workgroup
constexpr uint64_t kPivotTiedMaxG = 1u << 18;

// The class counts t0 / t1 / t2 (below, tied with, above the pivot) of `total` suffixes.
static int pivot_classes(Run& r, uint64_t total, const char* what, uint64_t t[3]) {
    SA_READ(ht, read_back(r.c, hw(kHwTotals).at, r.c->totals, 12, r.s));
    for (int k = 0; k < 3; ++k) t[k] = ht[k];
    if (t[0] + t[1] + t[2] != total)
        return set_err(SA_E_INTERNAL, "%spivot classes %llu + %llu + %llu != %llu", what, (unsigned long long)t[0],
                       (unsigned long long)t[1], (unsigned long long)t[2], (unsigned long long)total);
    return SA_OK;
}

// The tail both pivot rounds share.  The tied blocks' totals (m members and G
// groups that go to the next set, D heads) are read and range-checked ...
static int tied_totals(Run& r, uint64_t t1, uint64_t gmax, const char* what, SetTotals* tied) {
    SA_READ(hu, read_back(r.c, hw(kHwUTotals).at, r.c->totals + 4, 12, r.s));
    *tied = SetTotals{hu[2], hu[0], hu[1]};
    if (tied->m > t1 || tied->G > gmax || tied->D > gmax)
        return set_err(SA_E_INTERNAL, "%s %llu / %llu / %llu out of range", what, (unsigned long long)tied->m,
                       (unsigned long long)tied->G, (unsigned long long)tied->D);
    return SA_OK;
}
// ... and the rest's segments appended to set uo after them (*all: theirs in, the set's out)
template <class Pos>
static int rest_segments(Run& r, const SegSrc& rest, Pos pos, uint32_t* d_sa, int uo, SetTotals* all) {
    SegDest d;
    d.set_off = all->m;
    d.g_off = (uint32_t)all->G;
    d.gsn = r.c->u_gs[uo];
    SegResult sr;
    SA_TRY(segments(r, rest, pos, false, d_sa, uo, &sr, d));
    *all = sr.t + *all;
    return SA_OK;
}

// a doubling round's fixed facts, built once per round
struct PivotRound {
    uint64_t n, h;
    uint32_t wr;      // bits of a rank
    int ui, uo;       // the set sorted, the set written
    uint64_t m, G;    // the set's suffixes and groups
    Chunking cu;
    uint64_t *ukb0, *ukb1;
    uint32_t* d_sa;
};
// sorted = nullptr: the tied blocks turned out small (the caller sorts the
// whole set).  segs_done: a tied-block round ran its own segments (`next`: the
// next set's totals; gs_written: its group starts are in u_gs[uo]).
struct PivotOut {
    uint64_t* sorted = nullptr;
    uint32_t P = 0;
    bool segs_done = false;
    SetTotals next;
    bool gs_written = false;
};

// kbA: a free key buffer (the round-1 keys, dead with dense ranks); have_gs:
// the set's group starts are in u_gs[ui] (written with it by the previous round)
static int pivot_round(Run& r, const PivotRound& p, uint64_t* kbA, bool have_gs, PivotOut* out) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    const auto [n, h, wr, ui, uo, m, G, cu, ukb0, ukb1, d_sa] = p;
    *out = PivotOut{};
    // tied-block round: its scratch is ukb0 (free: the tied members skip the
    // sorted output) -- gs, pr, toff, tid, then the rest's values (3 x
    // m' <= 3 m / 2 words)
    const uint64_t scap = 2 * align_up(c->cap, 64);
    const uint64_t sbase = align_up(4 * G + 3, 64);
    const uint64_t ra_max = align_up(m / 2, 64);
    // tied blocks write the next set's group starts: u_gs is allocated here,
    // and a workspace too tight for it takes the split path (k_pivot_pass<2>,
    // no extra memory) instead of failing the build
    const bool tied = !(c->dbg & SA_DEBUG_NO_TIED) && G <= kPivotTiedMaxG && sbase + 3 * ra_max <= scap &&
                      gs_available(c, n);
    uint32_t* const scr = reinterpret_cast<uint32_t*>(ukb0);
    // keys + class counts in one pass when the set came with its group starts (sa_pivot.h MODE 1)
    const bool merged = tied && have_gs;
    uint32_t* const gs = merged ? c->u_gs[ui] : tied ? scr : c->u_pos[uo];   // G (+ 1) group starts
    uint32_t* const pr = (tied ? scr : gs) + G + 1;                          // G pivot ranks
    uint32_t* const gP = c->vals_alt;                 // 3 (G + 1): members of each class before each group
    uint32_t* const cc = c->hist;                     // 3 x chunks class counts, scanned in place
    const uint32_t Gu = (uint32_t)G;
    if (!merged) {
        r.begin(SA_K_PIVOT_KEYS);
        hipLaunchKernelGGL(k_pivot_keys,
                           dim3((uint32_t)std::min<uint64_t>((m + kBlock * kPkItems - 1) / (kBlock * kPkItems), 8192)),
                           dim3(kBlock), 0, s, (const uint32_t*)c->u_idx[ui], (const uint32_t*)c->u_g[ui], m,
                           (const uint32_t*)c->rank, n, h, wr, Gu, ukb1, gs, pr);
        r.end();
        r.bytes(SA_K_PIVOT_KEYS, 20 * m);
    }
    r.begin(SA_K_PIVOT_COUNT);
    if (merged) {
        // the group starts came with the set: keys built and classes counted
        // in one pass (MODE 1: k_pivot_keys + MODE 0)
        const PivotKeySrc ks{c->rank, n, h, ukb1, pr};
        hipLaunchKernelGGL(k_pivot_pass<1>, dim3(cu.chunks), dim3(kBlock), 0, s, (const uint64_t*)nullptr,
                           (const uint32_t*)c->u_idx[ui], (const uint32_t*)c->u_g[ui], cu, (const uint32_t*)gs,
                           (const uint32_t*)pr, Gu, wr, cc, gP, nullptr, nullptr, nullptr, nullptr, TiedOut{}, ks);
    } else {
        hipLaunchKernelGGL(k_pivot_pass<0>, dim3(cu.chunks), dim3(kBlock), 0, s, (const uint64_t*)ukb1,
                           (const uint32_t*)c->u_idx[ui], (const uint32_t*)c->u_g[ui], cu, (const uint32_t*)gs,
                           (const uint32_t*)pr, Gu, wr, cc, gP, nullptr, nullptr, nullptr, nullptr, TiedOut{});
    }
    hipLaunchKernelGGL(k_scan_rows, dim3(3), dim3(kBlock), 0, s, cc, cu.chunks, c->totals);
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_PIVOT_COUNT, merged ? 20 * m : 8 * m);
    uint64_t t[3];
    SA_TRY(pivot_classes(r, m, "", t));
    const uint64_t t1 = t[1], mr = t[0] + t[2];
    SA_TRACE("  round h=%llu: pivot split, tied %llu of %llu%s", (unsigned long long)h, (unsigned long long)t1,
             (unsigned long long)m, tied ? " (tied blocks to the next set)" : "");
    if (t1 * 2 < m) return SA_OK;   // mostly distinct keys: the full sort is cheaper
    r.begin(SA_K_PIVOT_WRITE);
    hipLaunchKernelGGL(k_pivot_gp, dim3((uint32_t)std::min<uint64_t>((G + kBlock) / kBlock, 8192)), dim3(kBlock), 0, s,
                       (const uint32_t*)gs, Gu, (const uint32_t*)cc, cu, (const uint32_t*)c->totals, gP);
    const uint64_t ra = align_up(mr, 64);
    uint32_t* const ridx = tied ? scr + sbase : c->u_idx[uo];
    if (tied) {
        // the next set's group starts go with it (the next pivot round's MODE 1;
        // u_gs allocated by gs_available above)
        uint32_t* const toff = scr + 2 * G + 1;
        uint32_t* const tid = toff + G + 1;
        hipLaunchKernelGGL(k_pivot_tied_scan, dim3(1), dim3(kBlock), 0, s, (const uint32_t*)gP, Gu, toff, tid,
                           c->totals + 4);
        const TiedOut to{c->u_pos[ui], toff, tid, c->rank, d_sa, c->u_pos[uo], c->u_idx[uo], c->u_g[uo], c->u_gs[uo]};
        hipLaunchKernelGGL(k_pivot_pass<3>, dim3(cu.chunks), dim3(kBlock), 0, s, (const uint64_t*)ukb1,
                           (const uint32_t*)c->u_idx[ui], (const uint32_t*)c->u_g[ui], cu, (const uint32_t*)gs,
                           (const uint32_t*)pr, Gu, wr, cc, gP, nullptr, nullptr, kbA, ridx, to);
    } else {
        hipLaunchKernelGGL(k_pivot_pass<2>, dim3(cu.chunks), dim3(kBlock), 0, s, (const uint64_t*)ukb1,
                           (const uint32_t*)c->u_idx[ui], (const uint32_t*)c->u_g[ui], cu, (const uint32_t*)gs,
                           (const uint32_t*)pr, Gu, wr, cc, gP, ukb0, c->vals_u, kbA, ridx, TiedOut{});
    }
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_PIVOT_WRITE, tied ? 12 * m + 16 * t1 + 12 * mr : 12 * m + 12 * m);
    SetTotals& tb = out->next;   // the tied blocks', then the whole next set's
    if (tied) SA_TRY(tied_totals(r, t1, G, "tied blocks", &tb));
    Sorted rest;
    if (mr > 0) {
        // the rest sorted by (2 g + [> pivot], rank): values in u_idx / u_g
        // of the next set (free until segments()) or the tied round's
        // scratch, keys through kbA and ukb1
        const uint32_t bits = bit_width(2 * G - 1) + wr;
        const uint32_t Pn = (bits + 7) / 8;
        uint32_t* const va = tied ? ridx + ra : c->u_g[uo];
        uint32_t* const vb = tied ? ridx + 2 * ra : c->u_idx[uo];
        uint32_t* vfinal = (Pn & 1u) ? va : vb;
        uint32_t* vother = (Pn & 1u) ? vb : va;
        SA_TRY(radix_sort(r, SrcKeys{kbA, ridx}, 12 * mr, plan_chunks(mr), bits, SortBufs{vfinal, vother, ukb1, kbA},
                          &rest, SortFlags{false, true}));
        r.begin(SA_K_SORT_U);
        const dim3 pg((uint32_t)std::min<uint64_t>((mr + kBlock - 1) / kBlock, 8192));
        if (tied)
            hipLaunchKernelGGL(k_pivot_place<true>, pg, dim3(kBlock), 0, s, (const uint64_t*)rest.keys,
                               (const uint32_t*)vfinal, mr, (const uint32_t*)gs, (const uint32_t*)gP, Gu, wr, nullptr,
                               nullptr, m, (const uint32_t*)c->u_pos[ui], c->vals_u);
        else
            hipLaunchKernelGGL(k_pivot_place<false>, pg, dim3(kBlock), 0, s, (const uint64_t*)rest.keys,
                               (const uint32_t*)vfinal, mr, (const uint32_t*)gs, (const uint32_t*)gP, Gu, wr, ukb0,
                               c->vals_u, m, nullptr, nullptr);
        r.end();
        SA_HIP(hipGetLastError());
        r.bytes(SA_K_SORT_U, tied ? 20 * mr : 24 * mr);
        if (tied)
            SA_TRY(rest_segments(r, SegSrc{rest.keys, vfinal, plan_chunks(mr)}, PosArray{c->vals_u}, d_sa, uo, &tb));
    }
    out->P = 1 + rest.passes;
    out->gs_written = out->segs_done = tied;
    out->sorted = ukb0;
    return SA_OK;
}

// Round 1 by the pivot split (sa_pivot.h, R1): when the LSD round 1 would
// run and at least half of all suffixes share the key of suffix 0 (a text of
// one repeated symbol, configs[4]: all but the last K), those form one tied
// block -- ranks and the next unsorted set written directly -- and only the
// rest is radix sorted (then segments() over it, SA positions around the
// block's gap).  segs_done = false (nothing written but the class counts)
// when fewer share it: the caller runs the LSD sort.
static int pivot_round1(Run& r, uint64_t n, uint32_t bits1, uint32_t* d_sa, PivotOut* out) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    *out = PivotOut{};
    const Chunking ch = plan_chunks(n);
    const uint64_t* keys = c->keys[1];
    uint32_t* const gs = c->u_pos[1];   // {0, n}: one group
    uint32_t* const toff = gs + 2;
    uint32_t* const tid = gs + 4;
    uint32_t* const gP = c->vals_alt;   // 3 x 2
    uint32_t* const cc = c->hist;       // 3 x chunks class counts
    uint32_t* hg = c->host_words + hw(kHwGsInit).at;
    hg[0] = 0;
    hg[1] = (uint32_t)n;
    SA_HIP(hipMemcpyAsync(gs, hg, 8, hipMemcpyHostToDevice, s));
    r.begin(SA_K_PIVOT_COUNT);
    hipLaunchKernelGGL((k_pivot_pass<0, true>), dim3(ch.chunks), dim3(kBlock), 0, s, keys, nullptr, nullptr, ch,
                       (const uint32_t*)gs, nullptr, 1u, 0u, cc, gP, nullptr, nullptr, nullptr, nullptr, TiedOut{});
    hipLaunchKernelGGL(k_scan_rows, dim3(3), dim3(kBlock), 0, s, cc, ch.chunks, c->totals);
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_PIVOT_COUNT, 8 * n);
    uint64_t t[3];
    SA_TRY(pivot_classes(r, n, "round-1 ", t));
    const uint64_t t0 = t[0], t1 = t[1], mr = t0 + t[2];
    SA_TRACE("  round 1: pivot split, tied %llu of %llu", (unsigned long long)t1, (unsigned long long)n);
    if (t1 * 2 < n) return SA_OK;
    // the rest: keys -> keys[0], values ping-pong in u_idx[1] / u_g[1] (the
    // next set goes to u_*[0]), key buffers keys_u / keys[0]
    uint64_t* const rk = c->keys[0];
    uint32_t* const ridx = c->u_idx[1];
    // the set's group starts, for round 2's MODE 1; without room for them
    // round 1 keeps the LSD sort (done = false: nothing written yet)
    if (!gs_available(c, n)) return SA_OK;
    r.begin(SA_K_PIVOT_WRITE);
    hipLaunchKernelGGL(k_pivot_gp, dim3(1), dim3(kBlock), 0, s, (const uint32_t*)gs, 1u, (const uint32_t*)cc, ch,
                       (const uint32_t*)c->totals, gP);
    hipLaunchKernelGGL(k_pivot_tied_scan, dim3(1), dim3(kBlock), 0, s, (const uint32_t*)gP, 1u, toff, tid,
                       c->totals + 4);
    const TiedOut to{nullptr, toff, tid, c->rank, d_sa, c->u_pos[0], c->u_idx[0], c->u_g[0], c->u_gs[0]};
    hipLaunchKernelGGL((k_pivot_pass<3, true>), dim3(ch.chunks), dim3(kBlock), 0, s, keys, nullptr, nullptr, ch,
                       (const uint32_t*)gs, nullptr, 1u, 0u, cc, gP, nullptr, nullptr, rk, ridx, to);
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_PIVOT_WRITE, 8 * n + 16 * t1 + 12 * mr);
    SA_TRY(tied_totals(r, t1, 1, "round-1 tied block", &out->next));
    Sorted rest;
    if (mr > 0) {
        const uint32_t Pn = (bits1 + 7) / 8;
        uint32_t* const vfinal = (Pn & 1u) ? c->u_g[1] : ridx;
        uint32_t* const vother = (Pn & 1u) ? ridx : c->u_g[1];
        SA_TRY(radix_sort(r, SrcKeys{rk, ridx}, 12 * mr, plan_chunks(mr), bits1, SortBufs{vfinal, vother, c->keys_u, rk},
                          &rest));
        SA_TRY(rest_segments(r, SegSrc{rest.keys, vfinal, plan_chunks(mr)}, PosGap{t0, t1}, d_sa, 0, &out->next));
    }
    out->gs_written = out->segs_done = true;
    out->P = 2 + rest.passes;
    return SA_OK;
}

struct Round1Plan {
    uint32_t sigma = 0, K = 0;   // alphabet size; symbols round 1 sorts by
    BucketPlan bp;
    bool bucketed = false;
    bool complete = true;   // false: the text's tail holds a byte the sample missed
};

// alphabet -> dense codes (host reads the 256-bit presence mask) -> the plan
// of round 1.  sampled: the mask of a sample of the text (sa_alpha.h)
// instead of a pass over all of it.
static int plan_round1(Run& r, const uint8_t* d_text, uint64_t n, const sa_opts* opts, bool sampled, Round1Plan* pl) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    uint32_t* h_alpha = c->host_words + hw(kHwAlpha).at;
    uint16_t* h_code = reinterpret_cast<uint16_t*>(c->host_words + hw(kHwCode).at);
    // the text's last bytes: the compact key layout's check (short_suffix_ties)
    const uint32_t tail_n = (uint32_t)std::min<uint64_t>(n, (uint64_t)kMaxK);
    uint8_t* h_tail = reinterpret_cast<uint8_t*>(c->host_words + hw(kHwTail).at);
    SA_HIP(hipMemsetAsync(c->alpha, 0, 8 * 4, s));
    r.begin(SA_K_ALPHABET);
    if (sampled) {
        const bool first4k = (c->dbg & SA_DEBUG_ALPHA_SAMPLE_SMALL) != 0;
        const uint64_t nb = alpha_text_blocks(n), ns = alpha_sample_blocks(n, first4k);
        hipLaunchKernelGGL(k_alphabet_sample, dim3((uint32_t)std::min<uint64_t>(ns, 2ull * (uint32_t)c->cus)),
                           dim3(kBlock), 0, s, d_text, n, nb, ns, c->alpha);
        r.bytes(SA_K_ALPHABET, alpha_sample_bytes(n, first4k));
    } else {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kBlock * 16 - 1) / (kBlock * 16), SA_ALPHA_GRID);
        hipLaunchKernelGGL(k_alphabet, dim3(grid), dim3(kBlock), 0, s, d_text, n, c->alpha);
        r.bytes(SA_K_ALPHABET, n);
    }
    r.end();
    SA_HIP(hipGetLastError());
    SA_HIP(hipMemcpyAsync(h_alpha, c->alpha, 8 * 4, hipMemcpyDeviceToHost, s));
    SA_HIP(hipMemcpyAsync(h_tail, d_text + (n - tail_n), tail_n, hipMemcpyDeviceToHost, s));
    SA_HIP(host_sync(s));
    // the tail's bytes belong to the mask; one the sample missed shows
    // before any pass that the sample is not the alphabet
    pl->complete = true;
    for (uint32_t t = 0; t < tail_n; ++t) {
        const uint32_t x = h_tail[t];
        if (!((h_alpha[x >> 5] >> (x & 31)) & 1u)) pl->complete = false;
        h_alpha[x >> 5] |= 1u << (x & 31);
    }
    uint32_t sigma = 0;
    for (int b = 0; b < 256; ++b) h_code[b] = ((h_alpha[b >> 5] >> (b & 31)) & 1u) ? (uint16_t)(++sigma) : 0;
    pl->sigma = sigma;
    SA_HIP(hipMemcpyAsync(c->code, h_code, 256 * 2, hipMemcpyHostToDevice, s));
    c->dna = sigma == 4 && h_code['A'] && h_code['C'] && h_code['G'] && h_code['T'];
    pl->K = choose_chars(sigma, n, opts ? opts->init_chars : 0);
    // round 1: sort every suffix by its first K symbols -- bucketed (two
    // global passes + per-window LDS sort) when the text allows it, else the
    // LSD sort of the packed key
    // the bucketed round sorts by min_chars symbols (an explicit K as given):
    // rounding K up to fill radix passes only serves the LSD round, and a
    // shorter key1 keeps its low bits narrow enough for the fixed-span local
    // sort and the per-XCD second pass (1 GiB alnum: K 8 -> 7, 16.05 -> 13.59
    // ms, profiles/r06_h_bench_alnum_k*.log; DNA, ascii127, byte256: the same K)
    const uint32_t Kb = (opts && opts->init_chars > 0) || sigma <= 1 ? pl->K : min_chars(sigma, n);
    BucketPlan& bp = pl->bp;
    BucketAsk ask;
    ask.round1 = opts ? opts->round1 : SA_ROUND1_AUTO;
    ask.radix = c->radix;
    // (tests: SA_DEBUG_BB17 / _BB18 widen the buckets of a small text; 0 in production)
    ask.bb_min = (c->dbg & SA_DEBUG_BB18) ? 18u : (c->dbg & SA_DEBUG_BB17) ? 17u : 0u;
    ask.cmp = (c->dbg & SA_DEBUG_NO_CMP) ? 0 : 1;
    bool bucketed = plan_bucketed(sigma, n, Kb, ask, &bp);
    ask.cmp = 0;
    if (bucketed && bp.bs.cmp && short_suffix_ties(h_tail, n, tail_n, h_code, sigma, bp.bs.s, bp.bs.R))
        bucketed = plan_bucketed(sigma, n, Kb, ask, &bp);
    ask.cmp = 2;
    // a non-power-of-two alphabet one bit short of packed first-pass items
    // (1 GiB alnum / ascii127: 65 bits) takes the E-only layout when the
    // text's last K suffixes pad apart (BucketSpec, sa_kernels.h)
    const bool force_eonly = (c->dbg & SA_DEBUG_EONLY) != 0;
    if (bucketed && bp.bs.cmp == 1 && ((sigma & (sigma - 1)) != 0 || force_eonly) &&
        !(c->dbg & SA_DEBUG_NO_EONLY)) {
        const uint32_t hb = bp.bs.bb - kLoBits;
        BucketPlan b2;
        if ((force_eonly || !plan_pk8(bp, hb, c->dbg, true)) && plan_bucketed(sigma, n, Kb, ask, &b2) &&
            (force_eonly || plan_pk8(b2, hb, c->dbg, true)) &&
            !short_suffix_ties(h_tail, n, tail_n, h_code, sigma, b2.bs.s, b2.bs.R, b2.K))
            bp = b2;
    }
    pl->bucketed = bucketed;
    return SA_OK;
}

// what the doubling rounds need of round 1 (pl.K, pl.bucketed: as it ran)
struct Round1Result {
    Round1Plan pl;
    Bucketed1 b1;                // the bucketed round's: ksh, fused, round2 (1 gave up, 2 finished the build)
    int kind = SA_ROUND1_LSD, alphabet = SA_ALPHABET_EXACT;
    uint64_t* keys1 = nullptr;   // the sorted round-1 keys (sparse ranks look ranks up in them)
    uint32_t P = 0;
    SetTotals t;
    bool sparse = false;
    bool gs_ok[2] = {false, false};   // the set's group starts are in u_gs[set] (pivot rounds' MODE 1)
};

// The alphabet from a sample (n >= kPadMinN; SA_DEBUG_ALPHA_SAMPLE_SMALL:
// any n), kept only when round 1 is then the bucketed one: its first pass
// stages every byte of the text and proves the sample (k_split_text,
// alpha_bad).  Every other plan (sigma <= 1, no bucket layout, a forced
// LSD round) takes the exact pass right here, having paid the sample and
// one more host round trip.  A sample the first pass refutes -- a symbol
// in none of the sampled blocks -- costs that pass and the second, and the
// build starts again with the exact alphabet, once.
static int round1(Run& r, const uint8_t* d_text, uint64_t n, uint32_t* d_sa, const sa_opts* opts, Round1Result* out) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    Round1Plan& pl = out->pl;
    Bucketed1& b1 = out->b1;
    bool sampled = !(c->dbg & SA_DEBUG_NO_ALPHA_SAMPLE) && (n >= kPadMinN || (c->dbg & SA_DEBUG_ALPHA_SAMPLE_SMALL)) &&
                   c->radix == 0 && (opts ? opts->round1 : SA_ROUND1_AUTO) != SA_ROUND1_LSD;
    bool refuted = false;
    for (;;) {
        SA_TRY(plan_round1(r, d_text, n, opts, sampled, &pl));
        if (sampled && !(pl.bucketed && pl.complete)) {
            SA_TRACE("packed: sampled alphabet (sigma=%u) not kept: %s", pl.sigma,
                     pl.complete ? "round 1 is not bucketed" : "the tail holds another symbol");
            sampled = false;
            continue;
        }
        c->samples_pending = false;
        if (!pl.bucketed) break;
        // (all 256 values in the sample: nothing left to prove)
        c->alpha_prove = sampled && pl.sigma < 256;
        c->alpha_refuted = false;
        Round1Opts o;
        o.want_round2 = true;
        const int rc = round1_bucketed(r, d_text, n, d_sa, pl.bp, full_range(pl.bp, n), o, &b1);
        c->alpha_prove = false;
        if (rc) return rc;
        if (c->alpha_refuted) {
            SA_TRACE("packed: the first pass met a symbol outside the sampled alphabet, again with the exact one");
            sampled = false;
            refuted = true;
            continue;
        }
        pl.bucketed = b1.done;
        out->t = b1.seg;
        if (b1.done) {
            out->keys1 = c->keys[0];
            out->P = 2;
            pl.K = pl.bp.K;
        }
        break;
    }
    out->alphabet = refuted ? SA_ALPHABET_REFUTED : sampled ? SA_ALPHABET_SAMPLED : SA_ALPHABET_EXACT;
    const uint64_t base = (uint64_t)pl.sigma + 1;
    const Chunking ch = plan_chunks(n);
    PivotOut p1;   // round 1 by the pivot split (pivot_round1)
    if (!pl.bucketed) {
        const uint32_t K = pl.K;
        const uint32_t bits1 = key_bits(base, K);
        SA_TRACE("packed: sigma=%u K=%u bits=%u", pl.sigma, K, bits1);
        uint64_t top = 1;   // B^(K-1)
        for (uint32_t t = 1; t < K; ++t) top *= base;
        if (c->radix == 0) SA_TRY(onesweep_prepare(c, s));
        r.begin(SA_K_PACK);
        hipLaunchKernelGGL(k_pack_text, dim3(ch.chunks), dim3(kBlock), 0, s, d_text, n, (const uint16_t*)c->code, ch,
                           base, top, K, c->keys[1], c->hist, c->radix == 0 ? (bits1 + 7) / 8 : 0u, os_ghist(c));
        r.end();
        SA_HIP(hipGetLastError());
        r.bytes(SA_K_PACK, 9 * n);
        if (c->radix == 0 && !(c->dbg & SA_DEBUG_NO_PIVOT) && n >= (1u << 16))
            SA_TRY(pivot_round1(r, n, bits1, d_sa, &p1));
        if (p1.segs_done) {
            out->t = p1.next;
            out->P = p1.P;
        } else {
            Sorted so;
            SA_TRY(radix_sort(r, SrcKeysIota{c->keys[1]}, 8 * n, ch, bits1,
                              SortBufs{d_sa, c->vals_alt, c->keys[0], c->keys[1]}, &so, SortFlags{true, false}));
            out->keys1 = so.keys;
            out->P = so.passes;
        }
    }
    out->kind = pl.bucketed ? SA_ROUND1_BUCKETED : p1.segs_done ? SA_ROUND1_PIVOT : SA_ROUND1_LSD;
    if (p1.segs_done) {   // pivot_round1 ran the segments (dense ranks)
        out->gs_ok[0] = true;
    } else if (pl.bucketed && b1.fused) {   // segments came with the local sort (sparse ranks)
        out->sparse = true;
    } else {
        SegDest d;
        d.gsn = gs_buf(c, n, 0);
        SegResult sr;
        SA_TRY(segments(r, SegSrc{out->keys1, d_sa, ch}, PosIdentity{}, true, nullptr, 0, &sr, d));
        out->t = sr.t;
        out->sparse = sr.sparse;
        out->gs_ok[0] = d.gsn != nullptr;
    }
    return SA_OK;
}

// the key1 samples RankLookup::sparse searches, before the first round
// that looks a rank up through them (round 1 left them out: SegOut::samples)
static int ensure_samples(Run& r, const uint8_t* d_text, uint64_t n, uint32_t* d_sa, const Round1Result& r1) {
    sa_context* const c = r.c;
    if (!c->samples_pending) return SA_OK;
    c->samples_pending = false;
    const uint32_t ksh = r1.b1.ksh;
    const uint64_t ns = (n + (1ull << ksh) - 1) >> ksh;
    const uint32_t g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((ns + kBlock - 1) / kBlock, 8192));
    r.begin(SA_K_SORT_U);
    hipLaunchKernelGGL(k_key1_samples, dim3(g), dim3(kBlock), 0, r.s, d_text, n, (const uint16_t*)c->code, r1.pl.bp.bs,
                       (const uint32_t*)d_sa, ksh, r1.keys1);
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_SORT_U, 12 * ns);
    return SA_OK;
}

// the doubling rounds over the set round 1 left; *D: the distinct suffixes after each
static int doubling_rounds(Run& r, const uint8_t* d_text, uint64_t n, uint32_t* d_sa, const Round1Result& r1, uint64_t* D) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    const uint32_t K = r1.pl.K;
    const bool sparse = r1.sparse, bucketed = r1.pl.bucketed;
    bool gs_ok[2] = {r1.gs_ok[0], r1.gs_ok[1]};
    int uo = 0;
    // later rounds sort in the two buffers that do not hold the round-1 keys
    uint64_t* ukb0 = r1.keys1 == c->keys[0] ? c->keys[1] : c->keys[0];
    uint64_t* ukb1 = c->keys_u;
    const RankLookup rl{c->rank, c->member, r1.keys1, d_text, (const uint16_t*)c->code, n, (uint64_t)r1.pl.sigma + 1, K,
                        bucketed ? 1u : 0u, r1.pl.bp.bs, bucketed ? c->segw + kBstartOff : nullptr, d_sa, r1.b1.ksh};
    auto samples = [&] { return sparse ? ensure_samples(r, d_text, n, d_sa, r1) : SA_OK; };
    const uint32_t wr = bit_width(n);   // rank values 0..n
    uint64_t m = r1.t.m, G = r1.t.G;
    for (uint64_t h = K; m > 0; h *= 2) {
        if (h >= 2 * n) return set_err(SA_E_INTERNAL, "doubling did not converge (h=%llu)", (unsigned long long)h);
        const uint32_t wg = G > 1 ? bit_width(G - 1) : 0;
        const uint32_t bits = wg + wr;
        if (bits > 64) return set_err(SA_E_INTERNAL, "key of %u bits", bits);
        const Chunking cu = plan_chunks(m);
        const int ui = uo;
        uo ^= 1;
        Sorted so;
        PivotOut pv;   // (segs_done: a tied-block pivot round ran its own segments)
        const uint32_t *u_idx = c->u_idx[ui], *u_g = c->u_g[ui];
        // f(the set's (group, rank[x + h]) key source), by the kind of its ranks
        auto with_src = [&](auto f) {
            return sparse ? f(SrcU<true>{u_idx, u_g, rl, h, wr}) : f(SrcU<false>{u_idx, u_g, rl, h, wr});
        };
        const SortBufs bufs{c->vals_u, c->vals_alt, ukb0, ukb1};
        // the first round after a bucketed round 1 with sparse ranks: the keys'
        // ranks as key1 of x + K from the text (SrcUKey1) when group id and
        // key1 + 1 fit 64 bits
        uint32_t kb1 = 0;
        if (bucketed && sparse && h == K && !(c->dbg & SA_DEBUG_NO_KEY1_ROUND)) kb1 = key1_bits(r1.pl.bp.bs);
        const bool key1_round = kb1 > 0 && kb1 + wg <= 64;
        if (c->radix == 0 && G > 0 && m <= kUsAvg * G) {
            // small groups on average: sort each group in registers, unless
            // one of them is larger than kUsLimit (then the radix sort below)
            if (!key1_round) SA_TRY(samples());
            // the keys first, one lane per suffix, then each group's lane sorts
            // them in place (ukb0 is read and written by that lane only)
            auto launch = [&] {
                const dim3 gk((uint32_t)std::min<uint64_t>((m + kBlock - 1) / kBlock, 65536));
                const dim3 gu((uint32_t)std::min<uint64_t>((m + kBlock - 1) / kBlock, 8192));
                auto keys = [&](auto src) {
                    hipLaunchKernelGGL(k_usort_keys<decltype(src)>, gk, dim3(kBlock), 0, s, src, m, ukb0);
                };
                if (key1_round) keys(SrcUKey1{u_idx, u_g, rl, h, kb1});
                else with_src(keys);
                hipLaunchKernelGGL(k_usort_small<SrcKeys>, gu, dim3(kBlock), 0, s, SrcKeys{ukb0, u_idx}, u_g, m, ukb0,
                                   c->vals_u, c->words + kUsFlagWord);
            };
            bool ok = false;
            SA_TRY(usort_try(r, launch, &ok));
            r.bytes(SA_K_SORT_U, 28 * m);
            if (ok) so = Sorted{ukb0, 1};
            SA_TRACE("  round h=%llu: per-group register sort %s", (unsigned long long)h,
                     ok ? "done" : "found a large group");
        }
        if (!so.keys && pivot_ok(c, m, G, wr, sparse)) {
            uint64_t* kbA = ukb0 == c->keys[0] ? c->keys[1] : c->keys[0];   // the round-1 keys: dead with dense ranks
            SA_TRY(pivot_round(r, PivotRound{n, h, wr, ui, uo, m, G, cu, ukb0, ukb1, d_sa}, kbA, gs_ok[ui], &pv));
            so = Sorted{pv.sorted, pv.P};
            if (pv.segs_done) gs_ok[uo] = pv.gs_written;
        }
        if (!so.keys && c->radix == 0) {
            SA_TRY(with_src([&](auto src) { return usort_radix(r, src, u_idx, m, bits, bufs, samples, &so); }));
        } else if (!so.keys) {
            SA_TRY(samples());
            SA_TRY(with_src([&](auto src) {
                return radix_sort(r, src, 12 * m, cu, bits, bufs, &so, SortFlags{false, true});
            }));
        }
        SetTotals next = pv.next;
        if (!pv.segs_done) {
            SegDest d;
            d.gsn = gs_buf(c, n, uo);
            SegResult sr;
            SA_TRY(segments(r, SegSrc{so.keys, c->vals_u, cu}, PosArray{c->u_pos[ui]}, false, d_sa, uo, &sr, d));
            next = sr.t;
            gs_ok[uo] = d.gsn != nullptr;
        }
        r.round_mark();
        *D = (n - m) + next.D;
        record_round(r.st, 0.f, *D, so.passes, m, 2 * h);
        SA_TRACE("  round h=%llu: sorted %llu, D=%llu unsorted=%llu groups=%llu", (unsigned long long)h,
                 (unsigned long long)m, (unsigned long long)*D, (unsigned long long)next.m, (unsigned long long)next.G);
        m = next.m;
        G = next.G;
    }
    return SA_OK;
}

static int build_packed(Run& r, const uint8_t* d_text, uint64_t n, uint32_t* d_sa, const sa_opts* opts) {
    sa_stats* const st = r.st;
    SA_TRY(ensure_u_capacity(r.c, n));
    r.round_mark();
    Round1Result r1;
    SA_TRY(round1(r, d_text, n, d_sa, opts, &r1));
    const uint32_t K = r1.pl.K;
    if (st) {
        st->alphabet = r1.alphabet;
        st->init_chars = (int32_t)K;
        st->sigma = (int32_t)r1.pl.sigma;
        st->round1 = r1.kind;
        st->sparse_ranks = r1.sparse ? 1 : 0;
    }
    uint64_t D = r1.t.D;
    if (r1.b1.round2 == 0) r.round_mark();   // (else made before the round-2 kernel)
    record_round(st, 0.f, D, r1.P, n, K);
    SA_TRACE("  round 1: D=%llu unsorted=%llu groups=%llu", (unsigned long long)D, (unsigned long long)r1.t.m,
             (unsigned long long)r1.t.G);
    if (r1.b1.round2 == 2) {
        // round 2 ordered every group by its next K symbols, no two members
        // tied: the SA is complete
        r.round_mark();
        D = n;
        record_round(st, 0.f, D, 1, r1.t.m, 2 * (uint64_t)K);
        SA_TRACE("  round h=%u: sorted %llu from the local sort's staging, D=%llu", K, (unsigned long long)r1.t.m,
                 (unsigned long long)D);
    } else {
        SA_TRY(doubling_rounds(r, d_text, n, d_sa, r1, &D));
    }
    if (D != n) return set_err(SA_E_INTERNAL, "finished with %llu groups for n=%llu", (unsigned long long)D,
                               (unsigned long long)n);
    return SA_OK;
}
