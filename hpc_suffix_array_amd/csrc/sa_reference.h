// sa_reference.h -- the reference schedule: manber_myers.c:88-125 round for
// round.  Included by sa_build.hip in namespace sa, after the sorts.
#pragma once

static int build_reference(Run& r, const uint8_t* d_text, uint64_t n, uint32_t* d_sa) {
    sa_context* const c = r.c;
    const hipStream_t s = r.s;
    int rc = SA_OK;
    const Chunking ch = plan_chunks(n);
    // first ranks: dense codes 1..sigma of the bytes present (the order of
    // manber_myers.c:90's text[i] + 1, so D_j and the round count are the
    // reference's; the first key spans 2 bit_width(sigma) bits, not 18)
    uint16_t* h_code = reinterpret_cast<uint16_t*>(c->host_words + hw(kHwCode).at);
    SA_HIP(hipMemsetAsync(c->alpha, 0, 8 * 4, s));
    r.begin(SA_K_ALPHABET);
    {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + kBlock * 16 - 1) / (kBlock * 16), SA_ALPHA_GRID);
        hipLaunchKernelGGL(k_alphabet, dim3(grid), dim3(kBlock), 0, s, d_text, n, c->alpha);
    }
    r.end();
    r.bytes(SA_K_ALPHABET, n);
    SA_READ(h_alpha, read_back(c, hw(kHwAlpha).at, c->alpha, 8 * 4, s));
    uint32_t sigma = 0;
    for (int b = 0; b < 256; ++b) h_code[b] = ((h_alpha[b >> 5] >> (b & 31)) & 1u) ? (uint16_t)(++sigma) : 0;
    SA_HIP(hipMemcpyAsync(c->code, h_code, 256 * 2, hipMemcpyHostToDevice, s));
    uint64_t D = sigma;   // ranks 1..sigma (manber_myers.c:94 sizes its bins for 256)
    const uint64_t perm_min = perm_min_n(c);
    const uint32_t ib = std::max<uint32_t>(1, bit_width(n - 1));   // index bits of a packed item
    bool used_perm = false;
    bool hist_ready = false;   // this round's first-digit counts came with the previous re-rank (or the init)
    r.begin(SA_K_INIT);
    {
        // round 1's first-digit counts per XCD queue with the ranks (k_init_rank_hist)
        const uint32_t w1 = bit_width(D);
        const bool packed1 = c->radix == 0 && 2 * w1 + ib <= 64;
        const LsdPlan pl1 = lsd_plan(2 * w1, packed1 ? ib : 0, lsd_max_bits(c));
        if (c->radix == 0 && lsd_xq_ok(c, n, pl1, packed1)) {
            const NextHist x = lsd_xq_span(n);
            SA_HIP(hipMemsetAsync(c->lsdx, 0, 8 * kLsdMaxRadix * 4, s));
            const uint64_t grid = std::min<uint64_t>((n + kBlock * 16 - 1) / (kBlock * 16), 4ull * (uint64_t)c->cus);
            hipLaunchKernelGGL(k_init_rank_hist, dim3((uint32_t)grid), dim3(kBlock), 0, s, d_text, n,
                               (const uint16_t*)c->code, c->rank, w1, pl1.shift[0] - (packed1 ? ib : 0u),
                               (1u << pl1.bits[0]) - 1u, x.qd, c->lsdx);
            hist_ready = true;
        } else {
            const uint64_t grid = std::min<uint64_t>((n + kBlock * 4 - 1) / (kBlock * 4), 4096);
            hipLaunchKernelGGL(k_init_rank_dense, dim3((uint32_t)grid), dim3(kBlock), 0, s, d_text, n,
                               (const uint16_t*)c->code, c->rank);
        }
    }
    r.end();
    SA_HIP(hipGetLastError());
    r.bytes(SA_K_INIT, 5 * n);
    if (r.st) r.st->sigma = (int32_t)sigma;

    r.round_mark();
    for (uint64_t h = 1;; h *= 2) {
        const uint32_t w = bit_width(D);          // ranks are 0..D
        // (key << ib | index) items while they fit 64 bits (onesweep only)
        const bool packed = c->radix == 0 && 2 * w + ib <= 64;
        SA_TRACE("reference round h=%llu D=%llu w=%u%s", (unsigned long long)h, (unsigned long long)D, w,
                 packed ? " packed" : "");
        SrcRank src{c->rank, n, h, w};
        Sorted so;
        if (c->radix == 0) {
            const LsdPlan pl = lsd_plan(2 * w, packed ? ib : 0, lsd_max_bits(c));
            rc = packed ? lsd_sort<true>(r, SrcRankPk{c->rank, n, h, w, ib}, n, pl, d_sa, c->vals_alt, &so, hist_ready)
                        : lsd_sort<false>(r, src, n, pl, d_sa, c->vals_alt, &so, hist_ready);
        } else {
            rc = radix_sort(r, src, 4 * n, ch, 2 * w, SortBufs{d_sa, c->vals_alt, c->keys[0], c->keys[1]}, &so);
        }
        if (rc) return rc;
        uint64_t* const sorted = so.keys;
        // the permutation's first level counts heads per tile of its own
        const bool use_perm = packed || n >= perm_min;
        const uint32_t ptiles = (uint32_t)((n + kPermTile - 1) / kPermTile);
        r.begin(SA_K_HEADS);
        if (use_perm)
            hipLaunchKernelGGL((k_tile_heads<kPermBlock, kPermItems>), dim3(ptiles), dim3(kPermBlock), 0, s,
                               (const uint64_t*)sorted, n, packed ? ib : 0u, perm_tile_off(c));
        else
            hipLaunchKernelGGL(k_heads, dim3(ch.chunks), dim3(kBlock), 0, s, sorted, ch, c->counts, 0u);
        r.end();
        r.begin(SA_K_HEADS_SCAN);
        if (use_perm)
            hipLaunchKernelGGL(k_scan_heads, dim3(1), dim3(kBlock), 0, s, perm_tile_off(c), ptiles, c->words);
        else
            hipLaunchKernelGGL(k_scan_heads, dim3(1), dim3(kBlock), 0, s, c->counts, ch.chunks, c->words);
        r.end();
        SA_HIP(hipGetLastError());
        r.bytes(SA_K_HEADS, 8 * n);
        r.bytes(SA_K_HEADS_SCAN, 8ull * ch.chunks);
        // (with the permutation re-rank's error word: the previous round's
        // placement is checked before this round's ranks are used)
        SA_READ(hwd, read_words(c, 4 * (kPermErrWord + 1), s));
        if (hwd[kLookbackWord]) return set_err(SA_E_INTERNAL, "radix look-back did not complete");
        if (used_perm && hwd[kPermErrWord])
            return set_err(SA_E_INTERNAL, "re-rank permutation lost a suffix (flags %u)", hwd[kPermErrWord]);
        const uint64_t Dn = hwd[kDWord];
        const bool done = (Dn == n);                  // manber_myers.c:113
        if (done && packed) {
            r.begin(SA_K_RERANK);
            hipLaunchKernelGGL(k_items_to_sa, dim3((uint32_t)std::min<uint64_t>((n + kBlock - 1) / kBlock, 8192)),
                               dim3(kBlock), 0, s, (const uint64_t*)sorted, n, ib, d_sa);
            r.end();
            SA_HIP(hipGetLastError());
            r.bytes(SA_K_RERANK, 12 * n);
        }
        hist_ready = false;
        if (!done) {
            if (use_perm) {
                used_perm = true;
                // the next round's first digit lies in rank[i + 2h] alone (its
                // width <= w'): the re-rank counts it per queue of that round's
                // LSD passes while it writes rank[] (no histogram read then)
                NextHist nh;
                if (c->radix == 0) {
                    const uint32_t w2 = bit_width(Dn);
                    const bool packed2 = 2 * w2 + ib <= 64;
                    const LsdPlan pl2 = lsd_plan(2 * w2, packed2 ? ib : 0, lsd_max_bits(c));
                    if (pl2.bits[0] <= w2 && lsd_xq_ok(c, n, pl2, packed2)) {
                        nh = lsd_xq_span(n);
                        nh.out = c->lsdx;
                        nh.mask = (1u << pl2.bits[0]) - 1u;
                        nh.h = 2 * h;
                        hist_ready = true;
                    }
                }
                SA_TRY(rerank_permute(r, sorted, d_sa, ch, packed ? ib : 0u, nh));
            } else {
                r.begin(SA_K_RERANK);
                hipLaunchKernelGGL(k_rerank, dim3(ch.chunks), dim3(kBlock), 0, s, sorted, (const uint32_t*)d_sa, ch,
                                   (const uint32_t*)c->counts, c->rank);
                r.end();
                SA_HIP(hipGetLastError());
                r.bytes(SA_K_RERANK, 16 * n);
            }
        }
        r.round_mark();
        record_round(r.st, 0.f, Dn, so.passes, n, 2 * h);   // (its time: Run::round_times)
        if (Dn > n || Dn == 0)
            return set_err(SA_E_INTERNAL, "distinct count %llu out of range", (unsigned long long)Dn);
        if (done) break;
        if (h > n) return set_err(SA_E_INTERNAL, "doubling did not converge (h=%llu)", (unsigned long long)h);
        D = Dn;
    }
    if (used_perm) {
        SA_READ(perr, read_word(c, kPermErrWord, s));
        if (*perr) return set_err(SA_E_INTERNAL, "re-rank permutation lost a suffix (flags %u)", *perr);
    }
    return SA_OK;
}
